// layout.hip — NCHW <-> NHWC conversions, fill, the ConvTranspose2d backward prep, and the materialised sources
// (per-pixel, LDS-tiled Up-block input, max-pool with argmax codes).
#include "halo_items.h"

namespace unet {

// ---- layout ---------------------------------------------------------------------------------------
template <typename T>
__global__ void nchw_to_nhwc_kernel(long long N, int C, int H, int W, const float* x, T* y) {
  const long long total = N * C * (long long)H * W;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c = e % C;
    const long long p = e / C;
    const long long hw = p % ((long long)H * W), n = p / ((long long)H * W);
    y[e] = from_f<T>(x[(n * C + c) * (long long)H * W + hw]);
  }
}
// ---- materialise a virtual source (max-pool / bilinear-up + pad / BN-ReLU / gate) as a plain NHWC
// tensor.  The conv and wgrad loaders then read it as a PLAIN source: their per-element transform
// (VALU beside the MFMAs) costs more than one streaming pass over the result.
template <typename T>
__global__ void materialize_kernel(const unet_src s, long long N, int H, int W, T* out) {
  constexpr int VEC = Vec<T>::N;
  const int CV = (s.C + VEC - 1) / VEC;
  const long long total = N * H * (long long)W * CV;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int cv = (int)(e % CV);
    long long t = e / CV;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    const long long n = t / H;
    float v[VEC];
    src_gather<T>(&s, 1, s.C, H, W, n, y, x, cv * VEC, v);
    T* o = out + ((n * H + y) * (long long)W + x) * s.C + cv * VEC;
    if ((s.C % VEC) == 0) {
      store_vec<T>(o, v);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (cv * VEC + j < s.C) o[j] = from_f<T>(v[j]);
    }
  }
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(long long N, int C, int H, int W, const T* x, const float* sc, const float* sf,
                                    int relu, float* y) {
  const long long total = N * C * (long long)H * W;
  const long long HW = (long long)H * W;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long hw = e % HW;
    const long long t = e / HW;
    const int c = t % C;
    const long long n = t / C;
    float v = to_f(x[(n * HW + hw) * C + c]);
    if (sc) v = __builtin_fmaf(v, sc[c], sf[c]);
    if (relu) v = fmaxf(v, 0.f);
    y[e] = v;
  }
}
// x * sigmoid(psi) materialised as NCHW fp32 (standalone AttentionGate output, layers.py:192)
template <typename T>
__global__ void gated_to_nchw_kernel(long long N, int C, int H, int W, const T* x, const float* sc, const float* sf,
                                     int relu, const float* p, const float* ab, float* y) {
  const long long total = N * C * (long long)H * W;
  const long long HW = (long long)H * W;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long hw = e % HW;
    const long long t = e / HW;
    const int c = t % C;
    const long long n = t / C;
    float v = __builtin_fmaf(to_f(x[(n * HW + hw) * C + c]), sc[c], sf[c]);
    if (relu) v = fmaxf(v, 0.f);
    y[e] = v * sigmoidf_(p[n * HW + hw] * ab[0] + ab[1]);
  }
}
__global__ void fill_kernel(float* x, long long n, float v) {
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) x[e] = v;
}

// ConvTranspose2d(k=2, s=2) backward prep: space-to-depth of the output gradient into the gradient of
// the equivalent 1x1 conv (channel (2a+b)*Ct + c), plus per-block bias partial sums.
// Block: CLN channel lanes x PL pixel lanes; one pixel range per block (fixed order -> deterministic).
constexpr int CT_MAXCH = 4;  // channel chunks of 256 per thread (Ct <= 1024)
template <typename T>
__global__ __launch_bounds__(256) void convt_bwd_prep_kernel(long long N, int h, int w, int Ct, int Hp, int Wp, int pt,
                                                             int pl, const float* d_up, T* out, float* partial,
                                                             int rows) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int CLN = Ct < 256 ? Ct : 256, PL = 256 / CLN;
  const int cl = tid % CLN, pq = tid / CLN;
  const long long P = N * h * w;
  const long long per = (P + rows - 1) / rows;
  const long long p0 = blockIdx.x * per, p1 = min(P, p0 + per);
  float bs[CT_MAXCH];
#pragma unroll
  for (int k = 0; k < CT_MAXCH; ++k) bs[k] = 0.f;
  if (pq < PL) {
    for (long long p = p0 + pq; p < p1; p += PL) {
      const int x = p % w;
      const long long t = p / w;
      const int y = t % h;
      const long long n = t / h;
#pragma unroll
      for (int k = 0; k < CT_MAXCH; ++k) {
        const int c = cl + k * CLN;
        if (c < Ct) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const long long src = ((n * Hp + pt + 2 * y + (q >> 1)) * (long long)Wp + pl + 2 * x + (q & 1)) * Ct + c;
            const float v = d_up[src];
            out[p * 4 * Ct + q * Ct + c] = from_f<T>(v);
            bs[k] += v;
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CT_MAXCH; ++k) {
    if (k * CLN >= Ct) break;
    red[tid] = (pq < PL) ? bs[k] : 0.f;
    __syncthreads();
    if (tid < CLN && cl + k * CLN < Ct) {
      float a = 0.f;
      for (int q = 0; q < PL; ++q) a += red[q * CLN + tid];
      partial[(size_t)blockIdx.x * Ct + cl + k * CLN] = a;
    }
    __syncthreads();
  }
}

// fast form (C % VEC == 0): e = pixel * CV + cv with cv fastest, so stores are coalesced and, since
// the grid stride is a multiple of CV (a power of two <= 256 here), every thread keeps one channel
// vector: its BN scale/shift are loaded once (make_view) and each pixel is one item_issue/finish
struct MatDesc {
  int nsrc;
  unet_src src[2];
  int Cin;
};

// I: the element index type — unsigned (32-bit division: ~10 VALU instead of a ~100-instruction 64-bit
// division sequence, of which there are four per element) whenever N*H*W*CV < 2^31 (host-chosen)
template <typename T, int RAW, typename I = unsigned>
__global__ void materialize_fast_kernel(const MatDesc d, long long N, int H, int W, T* out) {
  constexpr int VEC = Vec<T>::N;
  const int C = d.src[0].C;
  const int CV = C / VEC;
  const int cvs = __builtin_ctz(CV);   // CV is a power of two (host-checked)
  const I total = (I)(N * H * (long long)W * CV);
  const I stride = (I)gridDim.x * blockDim.x;
  I e = (I)blockIdx.x * blockDim.x + threadIdx.x;
  const int cv = (int)(e & (CV - 1));
  SrcView sv;
  float sc[VEC], sf[VEC];
  make_view<T>(d, cv * VEC, sv, sc, sf);
  for (; e < total; e += stride) {
    const I px = e >> cvs;
    const I t = px / (I)W;
    const int x = (int)(px - t * (I)W);
    const I t2 = t / (I)H;
    const int y = (int)(t - t2 * (I)H);
    const int n = (int)t2;
    Item<RAW> it;
    item_issue<T, RAW>(sv, H, W, n, y, x, 1, it);
    float v[VEC];
    item_finish<T, RAW>(d, sv, sc, sf, n, y, x, cv * VEC, it, v);
    store_vec<T>(out + (size_t)px * C + cv * VEC, v);
  }
}

// The Up block's decoder input (layers.py:98-102: bilinear x2 upsample, align_corners=True, of relu(BN(x1)), then
// F.pad to x2's size) as LDS tiles (round 5).  The per-pixel form above gathers the 4 bilinear taps of every output
// vector from L2 and runs the BN affine on each (4 x the reads and the affine work of the source it needs); here a
// block owns MUP_TJ output rows x MUP_TX output columns x MUP_CT channel vectors, stages the source rows / columns
// they touch once (<= MUP_TJ/2+2 x MUP_TX/2+2 for scales <= 1/2, host-checked) as fp32 activations in LDS, and
// blends each output from there — with the same tap indices, weights and fma order as item_issue / item_finish
// (mode 4), so the map is bit-identical to the per-pixel form and to the convs' virtual UP_ACT sources.
constexpr int MUP_TJ = 8, MUP_TX = 32, MUP_SJ = MUP_TJ / 2 + 2, MUP_SX = MUP_TX / 2 + 2, MUP_CT = 8;
template <typename T>
__global__ __launch_bounds__(256) void materialize_up_tile_kernel(const unet_src s, int H, int W, T* out) {
  typedef __attribute__((ext_vector_type(2))) float f2;
  __shared__ float4 tile[MUP_SJ * MUP_SX * MUP_CT * 2];   // 8 fp32 activations (2 float4) per source vector
  const int C = s.C, CV = C >> 3;
  const int CT = CV < MUP_CT ? CV : MUP_CT;               // a power of two: a thread keeps one channel vector
  const int tid = threadIdx.x, cv = tid & (CT - 1);
  const int tiles_h = (H + MUP_TJ - 1) / MUP_TJ;
  const int n = (int)blockIdx.y / tiles_h, oy0 = ((int)blockIdx.y - n * tiles_h) * MUP_TJ;
  const int ox0 = (int)blockIdx.x * MUP_TX;
  const int c = ((int)blockIdx.z * CT + cv) * 8;          // this thread's first channel
  // the up-region rows / columns the tile covers and the source span they read
  int ua = oy0 - s.pad_t, ub = oy0 + MUP_TJ - 1 - s.pad_t, va = ox0 - s.pad_l, vb = ox0 + MUP_TX - 1 - s.pad_l;
  ua = ua < 0 ? 0 : ua; ub = ub > s.up_h - 1 ? s.up_h - 1 : ub;
  va = va < 0 ? 0 : va; vb = vb > s.up_w - 1 ? s.up_w - 1 : vb;
  int sy0 = 0, sx0 = 0, ny = 0, nx = 0;
  if (ua <= ub && va <= vb) {
    int i0, i1;
    float l;
    lin_idx(s.sh, ua, s.H, i0, i1, l);
    sy0 = i0;
    lin_idx(s.sh, ub, s.H, i0, i1, l);
    ny = i1 - sy0 + 1;
    lin_idx(s.sw, va, s.W, i0, i1, l);
    sx0 = i0;
    lin_idx(s.sw, vb, s.W, i0, i1, l);
    nx = i1 - sx0 + 1;
    ny = ny < MUP_SJ ? ny : MUP_SJ;                        // (host-checked; a clamp keeps LDS in bounds regardless)
    nx = nx < MUP_SX ? nx : MUP_SX;
  }
  float sc[8], sf[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { sc[j] = s.scale[c + j]; sf[j] = s.shift[c + j]; }
  // phase 1: the source span -> LDS, BN affine (+ ReLU) in fp32 as item_finish applies it per tap
  const T* src = (const T*)s.data;
  for (int i = tid; i < ny * nx * CT; i += 256) {
    const int px = i / CT, sxr = px % nx, syr = px / nx;
    const unsigned pix = ((unsigned)n * s.H + (unsigned)(sy0 + syr)) * (unsigned)s.W + (unsigned)(sx0 + sxr);
    float t[8];
    unpack16<T>(*reinterpret_cast<const uint4*>(src + (size_t)pix * C + c), t);
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      f2 r = __builtin_elementwise_fma(f2{t[j], t[j + 1]}, f2{sc[j], sc[j + 1]}, f2{sf[j], sf[j + 1]});
      if (s.relu) r = f2{fmaxf(r[0], 0.f), fmaxf(r[1], 0.f)};
      a[j] = r[0];
      a[j + 1] = r[1];
    }
    float4* d4 = tile + ((syr * MUP_SX + sxr) * MUP_CT + cv) * 2;
    d4[0] = make_float4(a[0], a[1], a[2], a[3]);
    d4[1] = make_float4(a[4], a[5], a[6], a[7]);
  }
  __syncthreads();
  // phase 2: the outputs (zero outside the up region: F.pad)
  for (int i = tid; i < MUP_TJ * MUP_TX * CT; i += 256) {
    const int px = i / CT, oxr = px % MUP_TX, oyr = px / MUP_TX;
    const int oy = oy0 + oyr, ox = ox0 + oxr;
    if (oy >= H || ox >= W) continue;
    const int uy = oy - s.pad_t, ux = ox - s.pad_l;
    float v[8];
    if (uy >= 0 && uy < s.up_h && ux >= 0 && ux < s.up_w) {
      int y0, y1, x0, x1;
      float ly, lx;
      lin_idx(s.sh, uy, s.H, y0, y1, ly);
      lin_idx(s.sw, ux, s.W, x0, x1, lx);
      const float hy0 = 1.f - ly, wx0 = 1.f - lx;
      const float w0s = hy0 * wx0, w1s = hy0 * lx, w2s = ly * wx0, w3s = ly * lx;
      const f2 w0 = {w0s, w0s}, w1 = {w1s, w1s}, w2 = {w2s, w2s}, w3 = {w3s, w3s};
      const float4* r0 = tile + (((y0 - sy0) * MUP_SX + (x0 - sx0)) * MUP_CT + cv) * 2;
      const float4* r1 = tile + (((y0 - sy0) * MUP_SX + (x1 - sx0)) * MUP_CT + cv) * 2;
      const float4* r2 = tile + (((y1 - sy0) * MUP_SX + (x0 - sx0)) * MUP_CT + cv) * 2;
      const float4* r3 = tile + (((y1 - sy0) * MUP_SX + (x1 - sx0)) * MUP_CT + cv) * 2;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 a0 = r0[h], a1 = r1[h], a2 = r2[h], a3 = r3[h];
        const f2 p0 = __builtin_elementwise_fma(w3, f2{a3.x, a3.y}, __builtin_elementwise_fma(w2, f2{a2.x, a2.y},
                        __builtin_elementwise_fma(w1, f2{a1.x, a1.y}, w0 * f2{a0.x, a0.y})));
        const f2 p1 = __builtin_elementwise_fma(w3, f2{a3.z, a3.w}, __builtin_elementwise_fma(w2, f2{a2.z, a2.w},
                        __builtin_elementwise_fma(w1, f2{a1.z, a1.w}, w0 * f2{a0.z, a0.w})));
        v[4 * h] = p0[0]; v[4 * h + 1] = p0[1]; v[4 * h + 2] = p1[0]; v[4 * h + 3] = p1[1];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    store_vec<T>(out + ((size_t)((unsigned)n * H + oy) * W + ox) * C + c, v);
  }
}

// MaxPool2d(2) of relu?(scale*y + shift) with argmax codes; one thread per pooled channel vector
// (I as materialize_fast_kernel)
template <typename T, typename I = unsigned>
__global__ void materialize_pool_kernel(const unet_src s, long long N, int H, int W, T* out, uint8_t* code) {
  constexpr int VEC = Vec<T>::N;
  const int C = s.C, CV = C / VEC;
  const int cvs = __builtin_ctz(CV);
  const I total = (I)(N * H * (long long)W * CV);
  const I stride = (I)gridDim.x * blockDim.x;
  I e = (I)blockIdx.x * blockDim.x + threadIdx.x;
  const int cv = (int)(e & (CV - 1));
  float sc[VEC], sf[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sc[j] = s.scale[cv * VEC + j]; sf[j] = s.shift[cv * VEC + j]; }
  const float lo = s.relu ? 0.f : -INFINITY;
  for (; e < total; e += stride) {
    const I px = e >> cvs;
    const I t = px / (I)W;
    const int x = (int)(px - t * (I)W);
    const I t2 = t / (I)H;
    const int y = (int)(t - t2 * (I)H);
    const long long n = (long long)t2;
    float best[VEC];
    int arg[VEC];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[VEC];
      load_vec<T>((const T*)s.data + (((n * s.H + 2 * y + (q >> 1)) * (long long)s.W + 2 * x + (q & 1)) * C + cv * VEC), v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float r = __builtin_fmaf(v[j], sc[j], sf[j]);
        const float a = r != r ? r : fmaxf(r, lo);   // fmaxf drops a NaN; relu(NaN) is NaN
        if (q == 0 || a > best[j] || a != a) { best[j] = a; arg[j] = q; }
      }
    }
    store_vec<T>(out + (size_t)px * C + cv * VEC, best);
    unsigned lo4 = 0, hi4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) lo4 |= (unsigned)arg[j] << (8 * j);
    if constexpr (VEC == 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) hi4 |= (unsigned)arg[4 + j] << (8 * j);
      *reinterpret_cast<uint2*>(code + (size_t)px * C + cv * VEC) = make_uint2(lo4, hi4);
    } else {
      *reinterpret_cast<unsigned*>(code + (size_t)px * C + cv * VEC) = lo4;
    }
  }
}

// one launch per kernel, T from the entry point's dtype code (UNET_DISPATCH_T / _T16)
template <typename T>
static int launch_nchw_to_nhwc(hipStream_t st, long long N, int C, int H, int W, const float* x, void* y) {
  hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, dim3(grid_for(N * C * (long long)H * W, 8192)), dim3(256), 0, st, N, C, H, W,
                     x, (T*)y);
  return check_launch("nchw_to_nhwc");
}
template <typename T>
static int launch_nhwc_to_nchw(hipStream_t st, long long N, int C, int H, int W, const void* x, const float* sc,
                               const float* sf, int relu, float* y) {
  hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, dim3(grid_for(N * C * (long long)H * W, 8192)), dim3(256), 0, st, N, C, H, W,
                     (const T*)x, sc, sf, relu, y);
  return check_launch("nhwc_to_nchw");
}
template <typename T>
static int launch_gated_to_nchw(hipStream_t st, long long N, int C, int H, int W, const void* x, const float* sc,
                                const float* sf, int relu, const float* p, const float* ab, float* y) {
  hipLaunchKernelGGL(gated_to_nchw_kernel<T>, dim3(grid_for(N * C * (long long)H * W, 8192)), dim3(256), 0, st, N, C, H, W,
                     (const T*)x, sc, sf, relu, p, ab, y);
  return check_launch("gated_to_nchw");
}
template <typename T>
static int launch_convt_bwd_prep(int rows, hipStream_t st, long long N, int h, int w, int Ct, int Hp, int Wp, int pt,
                                 int pl, const float* d_up, void* out, float* partial) {
  hipLaunchKernelGGL(convt_bwd_prep_kernel<T>, dim3(rows), dim3(256), 0, st, N, h, w, Ct, Hp, Wp, pt, pl, d_up, (T*)out,
                     partial, rows);
  return check_launch("convt_bwd_prep");
}
template <typename T>
static int launch_mat_up_tile(dim3 grid, hipStream_t st, const unet_src& s, int H, int W, void* out) {
  hipLaunchKernelGGL(materialize_up_tile_kernel<T>, grid, dim3(256), 0, st, s, H, W, (T*)out);
  return check_launch("materialize up tile");
}
// I: the kernels' element index type
template <typename T, typename I>
static int launch_mat_fast(int raw, int blocks, hipStream_t st, const MatDesc& md, long long N, int H, int W, void* out) {
  if (raw == 4)
    hipLaunchKernelGGL((materialize_fast_kernel<T, 4, I>), dim3(blocks), dim3(256), 0, st, md, N, H, W, (T*)out);
  else
    hipLaunchKernelGGL((materialize_fast_kernel<T, 1, I>), dim3(blocks), dim3(256), 0, st, md, N, H, W, (T*)out);
  return check_launch("materialize");
}
template <typename T>
static int launch_mat(int blocks, hipStream_t st, const unet_src& s, long long N, int H, int W, void* out) {
  hipLaunchKernelGGL(materialize_kernel<T>, dim3(blocks), dim3(256), 0, st, s, N, H, W, (T*)out);
  return check_launch("materialize");
}
template <typename T, typename I>
static int launch_mat_pool(int blocks, hipStream_t st, const unet_src& s, long long N, int H, int W, void* out,
                           uint8_t* code) {
  hipLaunchKernelGGL((materialize_pool_kernel<T, I>), dim3(blocks), dim3(256), 0, st, s, N, H, W, (T*)out, code);
  return check_launch("materialize_pool");
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_nchw_to_nhwc(int dtype, long long N, int C, int H, int W, const float* x, void* y, void* stream) {
  return UNET_DISPATCH_T(dtype, launch_nchw_to_nhwc<T>((hipStream_t)stream, N, C, H, W, x, y));
}

int unet_nhwc_to_nchw(int dtype, long long N, int C, int H, int W, const void* x, const float* scale,
                      const float* shift, int relu, float* y, void* stream) {
  return UNET_DISPATCH_T(dtype, launch_nhwc_to_nchw<T>((hipStream_t)stream, N, C, H, W, x, scale, shift, relu, y));
}

int unet_gated_to_nchw(int dtype, long long N, int C, int H, int W, const void* x, const float* scale,
                       const float* shift, int relu, const float* p, const float* psi_ab, float* y, void* stream) {
  return UNET_DISPATCH_T(dtype,
                         launch_gated_to_nchw<T>((hipStream_t)stream, N, C, H, W, x, scale, shift, relu, p, psi_ab, y));
}

// the prep's partial rows follow OutConv's row policy (oc_rows, outconv.hip)
int unet_convt_bwd_rows(long long P) { return unet_outconv_rows(P); }

int unet_convt_bwd_prep(int dtype, long long N, int h, int w, int Ct, int Hp, int Wp, int pad_t, int pad_l,
                        const float* d_up, void* dy_s2d, float* partial, void* stream) {
  if (N <= 0 || h <= 0 || w <= 0 || Ct <= 0 || Ct > 256 * CT_MAXCH || pad_t < 0 || pad_l < 0 ||
      pad_t + 2 * h > Hp || pad_l + 2 * w > Wp) {
    set_error("unet_convt_bwd_prep: bad geometry");
    return UNET_ERR_ARG;
  }
  const int rows = unet_convt_bwd_rows(N * h * w);
  return UNET_DISPATCH_T(dtype, launch_convt_bwd_prep<T>(rows, (hipStream_t)stream, N, h, w, Ct, Hp, Wp, pad_t, pad_l,
                                                         d_up, dy_s2d, partial));
}

int unet_materialize(int dtype, const unet_src* src, long long N, int H, int W, void* out, void* stream) {
  if (!src || !out || N <= 0 || H <= 0 || W <= 0 || src->C <= 0 || !src->data || src->kind == UNET_SRC_NCHW_F32) {
    set_error("unet_materialize: bad arguments");
    return UNET_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int vec = dtype != UNET_F32 ? 8 : 4;
  const long long total = N * H * (long long)W * ((src->C + vec - 1) / vec);
  {
    // the tiled Up-block form: 16-bit, C/8 a power of two, both scales <= 1/2 (the span bound of its LDS tile);
    // UNET_MAT_TILE=0: the per-pixel form (A/B), read per call
    const char* e = getenv("UNET_MAT_TILE");
    const int cv8 = src->C / 8;
    if ((!e || atoi(e)) && dtype != UNET_F32 && src->kind == UNET_SRC_UP_ACT && src->C % 8 == 0 && (cv8 & (cv8 - 1)) == 0 &&
        src->scale && src->shift && src->sh <= 0.5f && src->sw <= 0.5f && src->sh >= 0.f && src->sw >= 0.f &&
        N * H <= (1LL << 30) && (double)N * H * W * src->C < 4294967296.0 &&
        (double)N * src->H * src->W * src->C < 4294967296.0) {
      const int ct = cv8 < MUP_CT ? cv8 : MUP_CT;
      const dim3 grid((unsigned)cdiv(W, MUP_TX), (unsigned)(N * cdiv(H, MUP_TJ)), (unsigned)(cv8 / ct));
      return UNET_DISPATCH_T16(dtype, launch_mat_up_tile<T>(grid, st, *src, H, W, out));
    }
  }
  // (total >= 1: the arguments were checked above)
  const int b = grid_for(total, block_cap("UNET_MAT_BLOCKS", 4096));
  const int cv = src->C / vec;
  // 32-bit gather offsets in item_issue: the source must stay below 4 GiB
  const double bytes = (double)N * src->H * src->W * src->C * (dtype != UNET_F32 ? 2 : 4);
  if (src->C % vec == 0 && cv <= 256 && (cv & (cv - 1)) == 0 && bytes < 4294967296.0) {
    MatDesc md;
    md.nsrc = 1;
    md.src[0] = *src;
    md.src[1] = *src;
    md.Cin = src->C;
    const int raw = (src->kind == UNET_SRC_POOL_ACT || src->kind == UNET_SRC_UP_ACT) ? 4 : 1;
    if (total < (1LL << 31)) return UNET_DISPATCH_T(dtype, launch_mat_fast<T, unsigned>(raw, b, st, md, N, H, W, out));
    return UNET_DISPATCH_T(dtype, launch_mat_fast<T, unsigned long long>(raw, b, st, md, N, H, W, out));
  }
  return UNET_DISPATCH_T(dtype, launch_mat<T>(b, st, *src, N, H, W, out));
}

int unet_materialize_pool(int dtype, const unet_src* src, long long N, int H, int W, void* out, uint8_t* code,
                          void* stream) {
  const int vec = dtype != UNET_F32 ? 8 : 4;
  const int cv = src ? src->C / vec : 0;
  if (!src || !out || !code || src->kind != UNET_SRC_POOL_ACT || !src->scale || !src->shift || src->C % vec ||
      cv > 256 || (cv & (cv - 1)) || src->H < 2 * H || src->W < 2 * W) {
    set_error("unet_materialize_pool: needs a POOL_ACT source with C/vec a power of two <= 256");
    return UNET_ERR_ARG;
  }
  const long long total = N * H * (long long)W * cv;
  long long b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  hipStream_t st = (hipStream_t)stream;
  if (total < (1LL << 31)) return UNET_DISPATCH_T(dtype, launch_mat_pool<T, unsigned>((int)b, st, *src, N, H, W, out, code));
  return UNET_DISPATCH_T(dtype, launch_mat_pool<T, unsigned long long>((int)b, st, *src, N, H, W, out, code));
}

int unet_fill_f32(float* x, long long n, float v, void* stream) {
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, n, v);
  return check_launch("fill");
}

}  // extern "C"
