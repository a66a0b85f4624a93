// outconv_mc.hip — OutConv for 9..16 classes on MFMA ("mc": multi-class): forward and backward.
//
// Reference: OutConv = nn.Conv2d(C, n_classes, kernel_size=1) with bias (unet/models/layers.py:109-123) and its
// convolution_backward.  outconv.hip serves n_classes <= 8 with per-class scalar / shuffle kernels whose register and
// shuffle cost grows with the class count; sixteen classes are exactly one MFMA row tile, so here the class axis
// sits on an MFMA dimension and the channel (forward) or pixel (weight gradient) reduction happens inside the
// matrix instruction.  One kernel serves every K in [9, 16]: class rows K..15 are zero weights and are never stored.
//
// Operand convention (the conv kernels', not outconv.hip's fp32 math): the activation is one fmaf(y, scale, shift) in
// fp32 (exact ReLU mask), clamped, then rounded to the operand type T; w and dl are rounded to T where they enter an
// MFMA; accumulation is fp32; db = Σ dl is summed from the unrounded fp32 dl.  In fp32 mode nothing is rounded
// (16x16x4 f32).
//
//  * forward  D[k][px] = Σ_c W[k][c]·act(y)[px][c]: A = weight fragments (converted once per workgroup into LDS in
//    fragment-major order: one conflict-free 16-byte read per lane and 32-channel chunk, the same code for C = 16
//    and for the 512-channel deep-supervision heads), B = the activation, one 16-byte NHWC load per lane (8
//    channels of one pixel) transformed in registers.  A wave owns 64 consecutive pixels per step as 4 MFMA column
//    tiles with pixel = base + 4·column + tile, so the accumulator lane ends with 4 classes x 4 consecutive pixels:
//    one 16-byte NCHW store per class (256-byte runs per class and instruction) when H·W % 4 == 0, per-pixel stores
//    with (n, hw) computed per pixel otherwise.  Waves are persistent over pixel groups and the y loads run a ring
//    of XD (group, chunk) steps ahead, across group boundaries, so the next group's loads are in flight during the
//    current group's epilogue.
//  * backward: one launch; workgroup r owns row r of the partial table and a contiguous pixel range, walked in
//    32-pixel tiles.  The dl tile (16 classes x 32 pixels) is loaded once with coalesced, individually guarded
//    4-byte loads (so image-straddling and misaligned tiles need no second path) and kept in LDS in the two
//    layouts its two products want; the activation tile is staged in LDS as T.  Tile t+1's global loads are in
//    registers while tile t is computed.
//      da[px][c] = Σ_k W[k][c]·dl[k][px]: A = Wᵀ fragments (16 channels x 16 classes, LDS), B = dl; 16x16x16 MFMA
//        for 16-bit (no padded k), 4 x 16x16x4 for fp32; the lane holds 4 consecutive channels of one pixel:
//        16-byte fp32 stores or read-modify-writes into NHWC da.
//      dW[k][c] = Σ_px dl[k][px]·a[px][c]: pixels along the MFMA k dimension; both operands come out of LDS with
//        the transposed read ds_read_b64_tr_b16 (16-bit, as pw.hip's wgrad) or a plain gather (fp32).  Wave w owns
//        the channel tiles w, w+4, ... for both products, so a dW element is summed by one wave over the workgroup's
//        whole range, in pixel order: no cross-wave sum, no atomics, bit-identical from run to run.
//    part[r][k][c] and db (row K, column k) are written in unet_outconv_bwd_finalize's layout.
#include "conv_common.h"

namespace unet {

constexpr int MC_MINK = 9, MC_MAXK = 16, MC_MINC = 16, MC_MAXC = 512;
constexpr int MC_PT = 32;        // backward: pixels per tile
constexpr int MC_DLS = 36;       // backward: fp32 dl tile row stride (floats): class rows land 4 banks apart
constexpr int MC_DTS = 48;       // backward: 16-bit dl^T tile row stride (elements): an odd multiple of 32 B

static inline bool mc_ok(int dtype, int C, int K) {
  return (dtype == UNET_F32 || dtype == UNET_BF16 || dtype == UNET_F16) && K >= MC_MINK && K <= MC_MAXK &&
         C % 8 == 0 && C >= MC_MINC && C <= MC_MAXC;
}

// ---- 8-channel items: one lane's slice of a 32-channel chunk ---------------------------------------------------
template <typename T> struct Raw8 { uint4 q; };                 // as loaded: 8 x 16-bit
template <> struct Raw8<float> { float4 lo, hi; };
template <typename T> struct Op8 { typename Mma<T>::frag f; };  // as an MFMA operand (one 16x16x32 for 16-bit)
template <> struct Op8<float> { float v[8]; };                  // eight 16x16x4 steps for fp32

template <typename T>
__device__ __forceinline__ Raw8<T> mc_ld8(const T* p, bool ok) {
  Raw8<T> r;
  if constexpr (sizeof(T) == 2) {
    r.q = make_uint4(0u, 0u, 0u, 0u);
    if (ok) r.q = *reinterpret_cast<const uint4*>(p);
  } else {
    r.lo = make_float4(0.f, 0.f, 0.f, 0.f);
    r.hi = r.lo;
    if (ok) {
      r.lo = *reinterpret_cast<const float4*>(p);
      r.hi = *reinterpret_cast<const float4*>(p + 4);
    }
  }
  return r;
}
template <typename T>
__device__ __forceinline__ void mc_unpack(const Raw8<T>& r, float* v) {
  if constexpr (sizeof(T) == 2) {
    unpack8_16<T>(r.q, v);
  } else {
    v[0] = r.lo.x; v[1] = r.lo.y; v[2] = r.lo.z; v[3] = r.lo.w;
    v[4] = r.hi.x; v[5] = r.hi.y; v[6] = r.hi.z; v[7] = r.hi.w;
  }
}
template <typename T>
__device__ __forceinline__ Op8<T> mc_pack(const float* v) {
  Op8<T> o;
  if constexpr (sizeof(T) == 2) {
    o.f = __builtin_bit_cast(typename Mma<T>::frag, pack8_16<T>(v));
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = v[j];
  }
  return o;
}
// relu?(y·scale + shift) of 8 channels, rounded to T; `plain`: no affine and no ReLU, the stored bits are the operand
template <typename T>
__device__ __forceinline__ Op8<T> mc_act(const Raw8<T>& r, bool plain, const float* sc, const float* sf, float lo) {
  if constexpr (sizeof(T) == 2) {
    if (plain) {
      Op8<T> o;
      o.f = __builtin_bit_cast(typename Mma<T>::frag, r.q);
      return o;
    }
  }
  float v[8];
  mc_unpack<T>(r, v);
  if (!plain) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaxf(__builtin_fmaf(v[j], sc[j], sf[j]), lo);
  }
  return mc_pack<T>(v);
}
template <typename T>
__device__ __forceinline__ f32x4 mc_mma8(const Op8<T>& a, const Op8<T>& b, f32x4 c) {
  if constexpr (sizeof(T) == 2) {
    return Mma<T>::mma(a.f, b.f, c);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) c = Mma<float>::mma(a.v[j], b.v[j], c);
    return c;
  }
}

// ---- 4-class items of the input gradient: k = 4·(lane >> 4) + j ------------------------------------------------
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
template <typename T> struct Op4;
template <> struct Op4<bf16> { bf16x4 f; };
template <> struct Op4<f16> { f16x4 f; };
template <> struct Op4<float> { float v[4]; };

template <typename T>
__device__ __forceinline__ Op4<T> mc_pack4(const float* v) {
  Op4<T> o;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o.f[j] = from_f<T>(v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = v[j];
  }
  return o;
}
__device__ __forceinline__ f32x4 mc_mma4(const Op4<bf16>& a, const Op4<bf16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(i16x4, a.f), __builtin_bit_cast(i16x4, b.f), c,
                                                   0, 0, 0);
}
__device__ __forceinline__ f32x4 mc_mma4(const Op4<f16>& a, const Op4<f16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(a.f, b.f, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mc_mma4(const Op4<float>& a, const Op4<float>& b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = Mma<float>::mma(a.v[j], b.v[j], c);
  return c;
}

// ------------------------------------------------------------------------------------------------
// forward.  LDS: weight fragments [nch][64] Op8<T>, then scale / shift [nch·32] (1 / 0 past C or when absent)
// ------------------------------------------------------------------------------------------------
template <typename T> __host__ __device__ constexpr int mc_xd() { return sizeof(T) == 2 ? 4 : 2; }

static inline size_t mc_fwd_lds(int esize, int C) {
  const size_t nch = (C + 31) / 32;
  return nch * 64 * (esize == 2 ? 16 : 32) + 2 * nch * 32 * sizeof(float);
}

template <typename T>
__global__ __launch_bounds__(256) void outconv_mc_fwd_kernel(long long P, int HW, int C, int K, const T* y,
                                                             const float* sc, const float* sf, int relu,
                                                             const float* w, const float* b, float* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mc_smem[];
  constexpr int XD = mc_xd<T>();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int nch = (C + 31) >> 5;
  Op8<T>* wl = reinterpret_cast<Op8<T>*>(mc_smem);
  float* ssc = reinterpret_cast<float*>(wl + nch * 64);
  float* ssf = ssc + nch * 32;
  // A fragments: lane (class i16, group g) of chunk ch holds W[i16][32·ch + 8·g + j]; zero rows / columns past K / C
  for (int i = tid; i < nch * 64; i += 256) {
    const int k = i & 15, c0 = (i >> 6) * 32 + ((i >> 4) & 3) * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (k < K && c0 + j < C) ? w[k * C + c0 + j] : 0.f;
    wl[i] = mc_pack<T>(v);
  }
  for (int i = tid; i < nch * 32; i += 256) {
    ssc[i] = (sc && i < C) ? sc[i] : 1.f;
    ssf[i] = (sf && i < C) ? sf[i] : 0.f;
  }
  __syncthreads();

  const bool plain = !sc && !sf && !relu;
  const float lo = relu ? 0.f : -INFINITY;
  const bool vec4 = (HW & 3) == 0;
  float bias[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bias[r] = (4 * g + r < K) ? b[4 * g + r] : 0.f;

  // pixel groups of 64; wave-persistent; steps (group, chunk) in order, the loads XD steps ahead
  const long long ngrp = (P + 63) >> 6, gstride = (long long)gridDim.x * 4;
  long long igrp = (long long)blockIdx.x * 4 + wave, cgrp = igrp;
  int ich = 0, cch = 0;
  Raw8<T> xq[XD][4];
  auto issue = [&](Raw8<T>* x) {
    if (igrp < ngrp) {
      const long long p = (igrp << 6) + 4 * i16;
      const int c8 = ich * 32 + 8 * g;   // channel groups past C read nothing: their addresses are the next pixel's
#pragma unroll
      for (int t = 0; t < 4; ++t) x[t] = mc_ld8<T>(y + (p + t) * C + c8, p + t < P && c8 < C);
    }
    if (++ich == nch) { ich = 0; igrp += gstride; }
  };
#pragma unroll
  for (int u = 0; u < XD; ++u) issue(xq[u]);

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  while (cgrp < ngrp) {
#pragma unroll
    for (int u = 0; u < XD; ++u) {
      if (cgrp < ngrp) {   // wave-uniform
        const Op8<T> wf = wl[cch * 64 + lane];
        float s8[8], f8[8];
        if (!plain) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { s8[j] = ssc[cch * 32 + 8 * g + j]; f8[j] = ssf[cch * 32 + 8 * g + j]; }
        }
        Op8<T> xb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) xb[t] = mc_act<T>(xq[u][t], plain, s8, f8, lo);
        issue(xq[u]);   // step + XD into the freed slot, ahead of the MFMAs and of the epilogue
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mc_mma8<T>(wf, xb[t], acc[t]);
        if (++cch == nch) {
          // lane: classes 4g + r, pixels p .. p + 3 (acc[t][r]: pixel p + t)
          const long long p = (cgrp << 6) + 4 * i16;
          if (vec4) {
            if (p < P) {   // P % 4 == 0: the four pixels are inside, in one image, 16-byte aligned
              const long long n = p / HW, hw = p - n * HW;
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (4 * g + r < K)
                  *reinterpret_cast<float4*>(out + (n * K + 4 * g + r) * HW + hw) =
                      make_float4(acc[0][r] + bias[r], acc[1][r] + bias[r], acc[2][r] + bias[r], acc[3][r] + bias[r]);
            }
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              if (p + t < P) {
                const long long n = (p + t) / HW, hw = (p + t) - n * HW;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (4 * g + r < K) out[(n * K + 4 * g + r) * HW + hw] = acc[t][r] + bias[r];
              }
            }
          }
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          cch = 0;
          cgrp += gstride;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward.  NT: channel tiles (of 16) per wave = 8-channel items per thread and tile = ceil(C / 64).
// LDS: Wᵀ fragments [nct][64] Op4<T> | scale, shift [16·nct] | a tile T [32][RS] | dl fp32 [16][MC_DLS] |
//      dlᵀ T [32][MC_DTS] (16-bit only)
// ------------------------------------------------------------------------------------------------
// a-tile row stride in elements: >= round_up(C, 16), an odd multiple of 32 bytes for the transposed 16-bit reads
static inline __host__ __device__ int mc_rs(int C) {
  const int c16 = (C + 15) & ~15;
  return ((c16 >> 4) & 1) ? c16 : c16 + 16;
}
static inline size_t mc_bwd_lds(int esize, int C) {
  const size_t nct = (C + 15) / 16;
  return nct * 64 * 4 * esize + 2 * nct * 16 * sizeof(float) + (size_t)MC_PT * mc_rs(C) * esize +
         16 * MC_DLS * sizeof(float) + (esize == 2 ? MC_PT * MC_DTS * 2 : 0);
}

template <typename T>
__device__ __forceinline__ typename Mma<T>::frag mc_tr8(const T* r0, const T* r1) {
  typedef __attribute__((ext_vector_type(8))) short i16x8;
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(r0));
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(r1));
  const i16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename Mma<T>::frag, r);
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void outconv_mc_bwd_kernel(long long P, int HW, int C, int K, const T* y,
                                                             const float* sc, const float* sf, int relu,
                                                             const float* w, const float* dl, float* da, int accum,
                                                             float* part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mc_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int nct = (C + 15) >> 4, RS = mc_rs(C), cv = C >> 3;
  Op4<T>* wt = reinterpret_cast<Op4<T>*>(mc_smem);
  float* ssc = reinterpret_cast<float*>(wt + nct * 64);
  float* ssf = ssc + nct * 16;
  T* at = reinterpret_cast<T*>(ssf + nct * 16);
  float* dlf = reinterpret_cast<float*>(at + MC_PT * RS);
  T* dlt = reinterpret_cast<T*>(dlf + 16 * MC_DLS);

  // A fragments of the input gradient: lane (channel i16 of tile ct, group g) holds W[4g + j][16·ct + i16]
  for (int i = tid; i < nct * 64; i += 256) {
    const int c = (i >> 6) * 16 + (i & 15), k0 = ((i >> 4) & 3) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (k0 + j < K && c < C) ? w[(k0 + j) * C + c] : 0.f;
    wt[i] = mc_pack4<T>(v);
  }
  for (int i = tid; i < nct * 16; i += 256) {
    ssc[i] = (sc && i < C) ? sc[i] : 1.f;
    ssf[i] = (sf && i < C) ? sf[i] : 0.f;
  }
  // columns C .. RS of the a tile feed only dW columns that are never written; zeroed once so they stay finite
  for (int i = tid; i < MC_PT * RS; i += 256) at[i] = from_f<T>(0.f);

  const bool plain = !sc && !sf && !relu;
  const float lo = relu ? 0.f : -INFINITY;
  const long long per = (P + gridDim.x - 1) / gridDim.x;
  const long long p0 = min(P, (long long)blockIdx.x * per), p1 = min(P, p0 + per);
  const int ntile = (int)((p1 - p0 + MC_PT - 1) / MC_PT);

  // this thread's y items (pixel row, 8-channel vector) and dl elements (class tid/32 + 8·e, pixel tid % 32) of a tile
  int ipx[NT], ic8[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int it = tid + 256 * k;
    ipx[k] = it / cv;
    ic8[k] = (it - ipx[k] * cv) * 8;
  }
  const int dpx = tid & 31, dk0 = tid >> 5;
  long long dn = (p0 + dpx) / HW;              // (n, hw) of this thread's dl pixel, advanced by 32 pixels per tile
  long long dhw = (p0 + dpx) - dn * HW;

  Raw8<T> yq[NT];
  float dq[2];
  auto issue = [&](int t) {
    const long long q0 = p0 + (long long)t * MC_PT;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const long long q = q0 + ipx[k];
      yq[k] = mc_ld8<T>(y + q * C + ic8[k], t < ntile && ipx[k] < MC_PT && q < p1);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = dk0 + 8 * e;
      dq[e] = (t < ntile && q0 + dpx < p1 && k < K) ? dl[(dn * K + k) * HW + dhw] : 0.f;
    }
    dhw += MC_PT;
    while (dhw >= HW) { dhw -= HW; ++dn; }
  };
  float dbs[2] = {0.f, 0.f};
  auto finish = [&]() {
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      if (ipx[k] < MC_PT) {
        float s8[8], f8[8];
        if (!plain) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { s8[j] = ssc[ic8[k] + j]; f8[j] = ssf[ic8[k] + j]; }
        }
        *reinterpret_cast<Op8<T>*>(at + ipx[k] * RS + ic8[k]) = mc_act<T>(yq[k], plain, s8, f8, lo);
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = dk0 + 8 * e;
      dlf[k * MC_DLS + dpx] = dq[e];
      if constexpr (sizeof(T) == 2) dlt[dpx * MC_DTS + k] = from_f<T>(dq[e]);
      dbs[e] += dq[e];   // db from the unrounded gradient
    }
  };

  f32x4 accw[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) accw[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  __syncthreads();   // the zeroed a tile, before the first finish writes into it
  issue(0);
  finish();
  __syncthreads();
  for (int t = 0; t < ntile; ++t) {
    issue(t + 1);
    const long long q0 = p0 + (long long)t * MC_PT;
    // ---- da: two 16-pixel column tiles x this wave's channel tiles
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = dlf[(4 * g + j) * MC_DLS + 16 * sub + i16];
      const Op4<T> bv = mc_pack4<T>(v);
      const long long q = q0 + 16 * sub + i16;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int ct = wave + 4 * i;
        if (ct < nct) {   // wave-uniform
          const f32x4 r = mc_mma4(wt[ct * 64 + lane], bv, f32x4{0.f, 0.f, 0.f, 0.f});
          const int c = 16 * ct + 4 * g;   // lane: channels c .. c + 3 of pixel q
          if (q < p1 && c < C) {
            float4* o = reinterpret_cast<float4*>(da + q * C + c);
            float4 s = make_float4(r[0], r[1], r[2], r[3]);
            if (accum) {
              const float4 old = *o;
              s.x += old.x; s.y += old.y; s.z += old.z; s.w += old.w;
            }
            *o = s;
          }
        }
      }
    }
    // ---- dW: pixels along k
    if constexpr (sizeof(T) == 2) {
      // tr-read geometry (pw.hip): lane (q4, p4) of a 16-lane group supplies row 8g + q4 (+ 4), columns p4 .. p4 + 3
      const int q4 = i16 >> 2, p4 = (i16 & 3) * 4;
      const int r0 = 8 * g + q4, r1 = r0 + 4;
      const typename Mma<T>::frag av = mc_tr8<T>(dlt + r0 * MC_DTS + p4, dlt + r1 * MC_DTS + p4);
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int ct = wave + 4 * i;
        if (ct < nct) {
          const typename Mma<T>::frag bv = mc_tr8<T>(at + r0 * RS + 16 * ct + p4, at + r1 * RS + 16 * ct + p4);
          accw[i] = Mma<T>::mma(av, bv, accw[i]);
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < MC_PT / 4; ++s) {
        const float av = dlf[i16 * MC_DLS + 4 * s + g];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const int ct = wave + 4 * i;
          if (ct < nct) accw[i] = Mma<float>::mma(av, (float)at[(4 * s + g) * RS + 16 * ct + i16], accw[i]);
        }
      }
    }
    __syncthreads();
    if (t + 1 < ntile) finish();
    __syncthreads();
  }

  // part[row][k][c]: accumulator rows are classes 4g + r, columns channels 16·ct + i16
  float* prow = part + (size_t)blockIdx.x * (K + 1) * C;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int c = 16 * (wave + 4 * i) + i16;
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < K) prow[(size_t)(4 * g + r) * C + c] = accw[i][r];
    }
  }
  // db: the 32 pixel columns of each class in a fixed order (dlf is free after the last barrier)
#pragma unroll
  for (int e = 0; e < 2; ++e) dlf[(dk0 + 8 * e) * MC_DLS + dpx] = dbs[e];
  __syncthreads();
  if (tid < K) {
    float s = 0.f;
    for (int j = 0; j < MC_PT; ++j) s += dlf[tid * MC_DLS + j];
    prow[(size_t)K * C + tid] = s;
  }
}

template <typename T, int NT>
static int mc_launch_bwd(int rows, size_t lds, hipStream_t st, long long P, int HW, int C, int K, const void* y,
                         const float* sc, const float* sf, int relu, const float* w, const float* dl, float* da,
                         int accum, float* part) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&outconv_mc_bwd_kernel<T, NT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("unet_outconv_mc_bwd: cannot reserve the LDS tile"); return (int)e; }
  }
  hipLaunchKernelGGL((outconv_mc_bwd_kernel<T, NT>), dim3(rows), dim3(256), lds, st, P, HW, C, K, (const T*)y, sc, sf,
                     relu, w, dl, da, accum, part);
  return check_launch("outconv_mc_bwd");
}

template <typename T>
static int mc_launch_fwd(int blocks, size_t lds, hipStream_t st, long long P, int HW, int C, int K, const void* y,
                         const float* sc, const float* sf, int relu, const float* w, const float* b, float* out) {
  hipLaunchKernelGGL(outconv_mc_fwd_kernel<T>, dim3(blocks), dim3(256), lds, st, P, HW, C, K, (const T*)y, sc, sf, relu,
                     w, b, out);
  return check_launch("outconv_mc_fwd");
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_outconv_mc_ok(int dtype, int C, int K) { return mc_ok(dtype, C, K) ? 1 : 0; }

int unet_outconv_mc_fwd(int dtype, long long N, int H, int W, int C, int K, const void* y, const float* scale,
                        const float* shift, int relu, const float* w, const float* b, float* logits, void* stream) {
  if (!mc_ok(dtype, C, K) || (scale == nullptr) != (shift == nullptr)) {
    set_error("unet_outconv_mc_fwd: needs 9 <= n_classes <= 16, C % 8 == 0, 16 <= C <= 512, scale and shift both or neither");
    return UNET_ERR_UNSUPPORTED;
  }
  const long long P = N * (long long)H * W;
  if (P <= 0 || (long long)H * W >= (1ll << 31)) { set_error("unet_outconv_mc_fwd: bad geometry"); return UNET_ERR_ARG; }
  const long long ngrp = (P + 63) / 64;
  long long blocks = (ngrp + 3) / 4;
  if (blocks > 1024) blocks = 1024;   // 4 workgroups per CU, persistent over the pixel groups
  const size_t lds = mc_fwd_lds(dtype == UNET_F32 ? 4 : 2, C);
  return UNET_DISPATCH_T(dtype, mc_launch_fwd<T>((int)blocks, lds, (hipStream_t)stream, P, H * W, C, K, y, scale, shift,
                                                 relu, w, b, logits));
}

int unet_outconv_mc_bwd(int dtype, long long N, int H, int W, int C, int K, const void* y, const float* scale,
                        const float* shift, int relu, const float* w, const float* dl, float* da, int accum,
                        float* part, void* stream) {
  if (!mc_ok(dtype, C, K) || (scale == nullptr) != (shift == nullptr)) {
    set_error("unet_outconv_mc_bwd: needs 9 <= n_classes <= 16, C % 8 == 0, 16 <= C <= 512, scale and shift both or neither");
    return UNET_ERR_UNSUPPORTED;
  }
  const long long P = N * (long long)H * W;
  if (P <= 0 || (long long)H * W >= (1ll << 31)) { set_error("unet_outconv_mc_bwd: bad geometry"); return UNET_ERR_ARG; }
  const int rows = unet_outconv_rows(P), HW = H * W;
  const size_t lds = mc_bwd_lds(dtype == UNET_F32 ? 4 : 2, C);
  hipStream_t st = (hipStream_t)stream;
  if (C <= 64)
    return UNET_DISPATCH_T(dtype, mc_launch_bwd<T, 1>(rows, lds, st, P, HW, C, K, y, scale, shift, relu, w, dl, da, accum, part));
  if (C <= 256)
    return UNET_DISPATCH_T(dtype, mc_launch_bwd<T, 4>(rows, lds, st, P, HW, C, K, y, scale, shift, relu, w, dl, da, accum, part));
  return UNET_DISPATCH_T(dtype, mc_launch_bwd<T, 8>(rows, lds, st, P, HW, C, K, y, scale, shift, relu, w, dl, da, accum, part));
}

}  // extern "C"
