// augment.hip — the device form of the reference's training augmentation chain (`get_train_transforms`,
// unet/data/augmentations.py:26-89) for a batch of decoded 8-bit slices.
//
// Every random decision is drawn on the host into one `unet_aug_params` row per sample
// (unet/utils/gpu_pipeline.py draw_train_augment); the kernels here are deterministic given that table:
//
//  * elastic_field: d = alpha * G_sigma * u for the samples whose elastic flag is set (a compact slot list).
//    u is i.i.d. uniform on [-1, 1) from Philox4x32-10, counter (pixel, stream, 0, 0), stream 1 = dx, 2 = dy,
//    keyed per sample; G_sigma is a separable normalised Gaussian of radius R with the reflect-101 border
//    (scipy gaussian_filter mode='mirror').  The horizontal pass generates its row segment and the 2R halo
//    straight into LDS (u is never stored), the vertical pass runs over LDS column tiles.
//  * augment_apply: one launch writes the fp32 NCHW image and the int64 mask.  The whole geometric chain is
//    ONE coordinate map per output pixel (grid distortion -> elastic -> inverse affine -> flips) followed by
//    one bilinear fetch of the resized u8 image (taps outside the frame are 0) and one nearest fetch of the
//    mask through the PIL NEAREST tables; then contrast/brightness, Gaussian noise (Philox stream 0),
//    coarse dropout and (v - mean) / std.  A sample without affine / elastic / grid takes the copy path:
//    integer (mirrored) source indices and image_finish_kernel's __fdiv_rn / __fsub_rn sequence, so an
//    all-off table reproduces unet_slice_finish bit for bit.
// HBM/L2-bound gathers; no MFMA.
#include "common.h"

namespace unet {

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2]
// ------------------------------------------------------------------------------------------------
struct u32x4 {
  unsigned x, y, z, w;
};

__device__ __forceinline__ u32x4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                               unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return u32x4{c0, c1, c2, c3};
}

// the elastic field's uniform on [-1, 1): exact in fp32
__device__ __forceinline__ float field_uniform(unsigned pixel, unsigned strm, unsigned k0, unsigned k1) {
  const unsigned w0 = philox4x32_10(pixel, strm, 0u, 0u, k0, k1).x;
  return __fsub_rn(__fmul_rn((float)(w0 >> 8), 0x1p-23f), 1.0f);
}

// a standard normal (Box-Muller) from the two first words of stream 0
__device__ __forceinline__ float noise_normal(unsigned pixel, unsigned k0, unsigned k1) {
  const u32x4 w = philox4x32_10(pixel, 0u, 0u, 0u, k0, k1);
  const float u1 = (float)((w.x >> 8) + 1u) * 0x1p-24f;   // (0, 1]
  const float u2 = (float)(w.y >> 8) * 0x1p-24f;          // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

__device__ __forceinline__ int reflect101(int i, int S) {  // one reflection: valid for -S < i < 2S - 1
  i = i < 0 ? -i : i;
  return i >= S ? 2 * (S - 1) - i : i;
}

// ------------------------------------------------------------------------------------------------
// elastic field
// ------------------------------------------------------------------------------------------------
constexpr int EF_TW = 256;   // horizontal pass: output columns per block (= threads)
constexpr int EF_TH = 64;    // vertical pass: output rows per block
constexpr int EF_TX = 64;    // vertical pass: columns per block (one wave wide: conflict-free LDS rows)
constexpr int EF_MAX_R = 96; // (EF_TH + 2R) * EF_TX * 4 B of LDS <= 64 KiB

// tmp[slot][comp][y][x] = sum_k taps[k] * u[y][reflect(x - R + k)];  grid (segments, S, 2 * n_slots)
__global__ void __launch_bounds__(EF_TW)
elastic_hblur_kernel(int S, int R, long long N, const unet_aug_params* __restrict__ table,
                     const int* __restrict__ slots, const float* __restrict__ taps, float* __restrict__ tmp) {
  extern __shared__ float lds[];   // [EF_TW + 2R]
  const int x0 = blockIdx.x * EF_TW, y = blockIdx.y;
  const int slot = blockIdx.z >> 1, comp = blockIdx.z & 1;
  const int n = slots[slot];
  const bool ok = n >= 0 && n < N;   // a slot list entry outside the table generates zeros
  const unsigned k0 = ok ? table[n].key[0] : 0u, k1 = ok ? table[n].key[1] : 0u;
  const int span = min(EF_TW, S - x0) + 2 * R;
  for (int i = threadIdx.x; i < span; i += EF_TW) {
    const int xs = reflect101(x0 - R + i, S);
    lds[i] = ok ? field_uniform((unsigned)(y * S + xs), 1u + comp, k0, k1) : 0.f;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= S) return;
  float acc = 0.f;
  for (int k = 0; k <= 2 * R; ++k) acc += taps[k] * lds[threadIdx.x + k];
  tmp[(((long long)slot * 2 + comp) * S + y) * S + x] = acc;
}

// field[slot][comp][y][x] = alpha * sum_k taps[k] * tmp[reflect(y - R + k)][x];  grid (col tiles, row tiles, 2 * n_slots)
__global__ void __launch_bounds__(256)
elastic_vblur_kernel(int S, int R, float alpha, const float* __restrict__ taps, const float* __restrict__ tmp,
                     float* __restrict__ field) {
  extern __shared__ float lds[];   // [EF_TH + 2R][EF_TX]
  const int x = blockIdx.x * EF_TX + (threadIdx.x & (EF_TX - 1));
  const int y0 = blockIdx.y * EF_TH;
  const int ty = threadIdx.x / EF_TX;   // 0..3
  const float* src = tmp + (long long)blockIdx.z * S * S;
  float* dst = field + (long long)blockIdx.z * S * S;
  const int rows = min(EF_TH, S - y0);
  const int span = rows + 2 * R;
  for (int i = ty; i < span; i += 256 / EF_TX) {
    const int ys = reflect101(y0 - R + i, S);
    lds[i * EF_TX + (threadIdx.x & (EF_TX - 1))] = x < S ? src[(long long)ys * S + x] : 0.f;
  }
  __syncthreads();
  if (x >= S) return;
  for (int r = ty; r < rows; r += 256 / EF_TX) {
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc += taps[k] * lds[(r + k) * EF_TX + (threadIdx.x & (EF_TX - 1))];
    dst[(long long)(y0 + r) * S + x] = alpha * acc;
  }
}

// ------------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------------
constexpr unsigned AUG_GEOMETRIC = UNET_AUG_AFFINE | UNET_AUG_ELASTIC | UNET_AUG_GRID;

// piecewise-linear knot table: output knots at k * S / 5, source knots g[0..5]
__device__ __forceinline__ float grid_map(const float* g, int x, int S, float cell) {
  const int k = min(5 * x / S, 4);
  const float t = ((float)x - (float)k * cell) / cell;
  return g[k] + t * (g[k + 1] - g[k]);
}

// bilinear fetch of one displacement component at (qx, qy), coordinates clamped to the frame
__device__ __forceinline__ float field_fetch(const float* __restrict__ f, int S, float qx, float qy) {
  const float cx = fminf(fmaxf(qx, 0.f), (float)(S - 1)), cy = fminf(fmaxf(qy, 0.f), (float)(S - 1));
  const int x0 = (int)floorf(cx), y0 = (int)floorf(cy);
  const int x1 = min(x0 + 1, S - 1), y1 = min(y0 + 1, S - 1);
  const float fx = cx - (float)x0, fy = cy - (float)y0;
  const float a = f[(long long)y0 * S + x0], b = f[(long long)y0 * S + x1];
  const float c = f[(long long)y1 * S + x0], d = f[(long long)y1 * S + x1];
  const float top = a + fx * (b - a), bot = c + fx * (d - c);
  return top + fy * (bot - top);
}

__device__ __forceinline__ float tap255(const unsigned char* __restrict__ img, int S, int x, int y) {
  return ((unsigned)x < (unsigned)S && (unsigned)y < (unsigned)S) ? __fdiv_rn((float)img[(long long)y * S + x], 255.0f) : 0.f;
}

// One thread per VEC consecutive pixels of a row (VEC = 4 when S % 4 == 0 and the outputs are 16-byte aligned:
// one float4 and two 16-byte mask stores).  n comes from blockIdx alone, so every table[n] read below is
// wave-uniform: the compiler keeps the row in scalar registers, loaded once per wave, not per pixel.
template <int VEC>
__global__ void __launch_bounds__(256)
augment_apply_kernel(long long N, int S, const unsigned char* __restrict__ img, int mask_h, int mask_w,
                     const unsigned char* __restrict__ mask, const int* __restrict__ ytab,
                     const int* __restrict__ xtab, const unet_aug_params* __restrict__ table,
                     const float* __restrict__ field, int n_elastic, float mean, float stdv,
                     float* __restrict__ out_img, int64_t* __restrict__ out_mask, int blocks_per_sample) {
  const long long n = blockIdx.x / blocks_per_sample;
  const int items = S * (S / VEC);
  const int e = (blockIdx.x % blocks_per_sample) * 256 + threadIdx.x;
  if (n >= N || e >= items) return;
  const unet_aug_params* __restrict__ p = table + n;
  const unsigned flags = p->flags;
  const int y = e / (S / VEC), xb = (e % (S / VEC)) * VEC;
  const unsigned char* src = img + n * S * S;
  const unsigned char* msrc = mask ? mask + n * mask_h * mask_w : nullptr;
  const bool hflip = flags & UNET_AUG_HFLIP, vflip = flags & UNET_AUG_VFLIP;
  const int slot = p->elastic_slot;
  const bool elastic = (flags & UNET_AUG_ELASTIC) && field && slot >= 0 && slot < n_elastic;
  const float last = (float)(S - 1), cell = (float)S / 5.0f;
  const int holes = (flags & UNET_AUG_DROPOUT) ? min(max(p->n_holes, 0), 4) : 0;

  float v[VEC];
  long long m[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int x = xb + j;
    if (!(flags & AUG_GEOMETRIC)) {   // copy path (wave-uniform branch): integer, possibly mirrored, source
      const int sx = hflip ? S - 1 - x : x, sy = vflip ? S - 1 - y : y;
      v[j] = __fdiv_rn((float)src[(long long)sy * S + sx], 255.0f);
      m[j] = msrc ? (msrc[(long long)ytab[sy] * mask_w + xtab[sx]] > 127 ? 1 : 0) : 0;
    } else {
      float cx = (float)x, cy = (float)y;
      if (flags & UNET_AUG_GRID) {
        cx = grid_map(p->gx, x, S, cell);
        cy = grid_map(p->gy, y, S, cell);
      }
      if (elastic) {
        const float* f = field + (long long)slot * 2 * S * S;
        const float dx = field_fetch(f, S, cx, cy), dy = field_fetch(f + (long long)S * S, S, cx, cy);
        cx += dx;
        cy += dy;
      }
      if (flags & UNET_AUG_AFFINE) {
        const float ax = p->inv_affine[0] * cx + p->inv_affine[1] * cy + p->inv_affine[2];
        const float ay = p->inv_affine[3] * cx + p->inv_affine[4] * cy + p->inv_affine[5];
        cx = ax;
        cy = ay;
      }
      if (vflip) cy = last - cy;
      if (hflip) cx = last - cx;
      // image: bilinear, taps outside the frame are 0 (the float -> int conversions saturate)
      const float fx0 = floorf(cx), fy0 = floorf(cy);
      const float fx = cx - fx0, fy = cy - fy0;
      const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)S), y0 = (int)fminf(fmaxf(fy0, -2.f), (float)S);
      const float a = tap255(src, S, x0, y0), b = tap255(src, S, x0 + 1, y0);
      const float c = tap255(src, S, x0, y0 + 1), d = tap255(src, S, x0 + 1, y0 + 1);
      const float top = a + fx * (b - a), bot = c + fx * (d - c);
      v[j] = top + fy * (bot - top);
      // mask: nearest
      const int ix = (int)fminf(fmaxf(floorf(cx + 0.5f), -1.f), (float)S);
      const int iy = (int)fminf(fmaxf(floorf(cy + 0.5f), -1.f), (float)S);
      const bool in = (unsigned)ix < (unsigned)S && (unsigned)iy < (unsigned)S;
      m[j] = (msrc && in) ? (msrc[(long long)ytab[iy] * mask_w + xtab[ix]] > 127 ? 1 : 0) : 0;
    }
    if (flags & UNET_AUG_BRIGHTNESS) v[j] = fminf(fmaxf(p->contrast * v[j] + p->brightness, 0.f), 1.f);
    if (flags & UNET_AUG_NOISE) {
      const float g = noise_normal((unsigned)(y * S + x), p->key[0], p->key[1]);
      v[j] = fminf(fmaxf(v[j] + p->noise_sigma * g, 0.f), 1.f);
    }
    for (int h = 0; h < holes; ++h)
      if (x >= p->holes[h][0] && y >= p->holes[h][1] && x < p->holes[h][2] && y < p->holes[h][3]) v[j] = 0.f;
    v[j] = __fdiv_rn(__fsub_rn(v[j], mean), stdv);
  }
  const long long o = (n * S + y) * S + xb;
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(out_img + o) = make_float4(v[0], v[1], v[2], v[3]);
    if (out_mask) {
      longlong2* mo = reinterpret_cast<longlong2*>(out_mask + o);
      mo[0] = make_longlong2(m[0], m[1]);
      mo[1] = make_longlong2(m[2], m[3]);
    }
  } else {
    out_img[o] = v[0];
    if (out_mask) out_mask[o] = m[0];
  }
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_aug_elastic_field(int n_slots, int S, float alpha, int R, const float* taps, long long N,
                           const unet_aug_params* table, const int32_t* slots, float* tmp, float* field,
                           void* stream) {
  if (n_slots <= 0 || n_slots > 32767 || S <= 0 || S > 32768 || R < 0 || N <= 0 || !taps || !table || !slots ||
      !tmp || !field) {
    set_error("unet_aug_elastic_field: bad arguments");
    return UNET_ERR_ARG;
  }
  if (S <= R) {   // one reflection must reach every halo index
    set_error("unet_aug_elastic_field: img_size must exceed the Gaussian radius int(4 * sigma + 0.5)");
    return UNET_ERR_ARG;
  }
  if (R > EF_MAX_R) {
    set_error("unet_aug_elastic_field: Gaussian radius above 96 (sigma > 24) is not supported");
    return UNET_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(elastic_hblur_kernel, dim3(cdiv(S, EF_TW), S, 2 * n_slots), dim3(EF_TW),
                     (size_t)(EF_TW + 2 * R) * sizeof(float), st, S, R, N, table, slots, taps, tmp);
  if (int rc = check_launch("elastic_hblur")) return rc;
  hipLaunchKernelGGL(elastic_vblur_kernel, dim3(cdiv(S, EF_TX), cdiv(S, EF_TH), 2 * n_slots), dim3(256),
                     (size_t)(EF_TH + 2 * R) * EF_TX * sizeof(float), st, S, R, alpha, taps, tmp, field);
  return check_launch("elastic_vblur");
}

int unet_aug_apply(long long N, int S, const uint8_t* img, int mask_h, int mask_w, const uint8_t* mask,
                   const int32_t* ytab, const int32_t* xtab, const unet_aug_params* table, long long table_len,
                   const float* field, int n_elastic, float mean, float stdv, float* out_img, int64_t* out_mask,
                   void* stream) {
  if (N <= 0 || S <= 0 || S > 32768 || !img || !table || !out_img || n_elastic < 0 || (n_elastic > 0 && !field) ||
      (mask && (!out_mask || mask_h <= 0 || mask_w <= 0 || !ytab || !xtab))) {
    set_error("unet_aug_apply: bad arguments");
    return UNET_ERR_ARG;
  }
  if (table_len != N) {
    set_error("unet_aug_apply: the parameter table must hold one row per image");
    return UNET_ERR_ARG;
  }
  const bool vec4 = (S % 4 == 0) && ((uintptr_t)out_img % 16 == 0) && ((uintptr_t)out_mask % 16 == 0);
  const long long items = (long long)S * (S / (vec4 ? 4 : 1));
  const int bps = cdiv(items, 256);
  if (N * bps > 0x7fffffffLL) {
    set_error("unet_aug_apply: batch too large for one launch");
    return UNET_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (vec4)
    hipLaunchKernelGGL(augment_apply_kernel<4>, dim3((unsigned)(N * bps)), dim3(256), 0, st, N, S, img, mask_h, mask_w,
                       mask, ytab, xtab, table, field, n_elastic, mean, stdv, out_img, out_mask, bps);
  else
    hipLaunchKernelGGL(augment_apply_kernel<1>, dim3((unsigned)(N * bps)), dim3(256), 0, st, N, S, img, mask_h, mask_w,
                       mask, ytab, xtab, table, field, n_elastic, mean, stdv, out_img, out_mask, bps);
  return check_launch("augment_apply");
}

}  // extern "C"
