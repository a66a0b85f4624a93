// upsample_bwd.hip — the adjoint of the bilinear upsample (per-element, windowed, LDS-tiled, and tiled with the attention
// gate's W_g 1x1 input gradient fused in) and the fp32 NCHW resize pair of the deep-supervision heads.
#include "halo_items.h"

namespace unet {

// sum over destination indices u in [0, up) whose interpolation touches source index i
// (weight (1-l) on i0, l on i1 — PyTorch's linear rule, align_corners=True)
__device__ __forceinline__ void up_range(float scale, int i, int in_size, int up, int& lo, int& hi) {
  if (scale > 0.f) {
    lo = (int)floorf((float)(i - 1) / scale) - 1;
    hi = (int)ceilf((float)(i + 1) / scale) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > up - 1 ? up - 1 : hi;
  } else {
    lo = 0;
    hi = up - 1;
  }
}
__device__ __forceinline__ float up_weight(float scale, int u, int in_size, int i) {
  int i0, i1;
  float l;
  lin_idx(scale, u, in_size, i0, i1, l);
  return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

// 4-channel vectorised form (C % 4 == 0): the index/weight arithmetic is shared by 4 channels
__global__ void upsample_bwd4_kernel(long long N, int C, int Hs, int Ws, int up_h, int up_w, int pt, int pl, int Hp,
                                     int Wp, float sh, float sw, const float* dup, float* dx, int accum) {
  const int C4 = C / 4;
  const long long total = N * Hs * (long long)Ws * C4;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c4 = e % C4;
    long long t = e / C4;
    const int j = t % Ws;
    t /= Ws;
    const int i = t % Hs;
    const long long n = t / Hs;
    int ulo, uhi, vlo, vhi;
    up_range(sh, i, Hs, up_h, ulo, uhi);
    up_range(sw, j, Ws, up_w, vlo, vhi);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int u = ulo; u <= uhi; ++u) {
      const float wy = up_weight(sh, u, Hs, i);
      const int yy = u + pt;
      if (wy == 0.f || yy < 0 || yy >= Hp) continue;
      const float4* row = reinterpret_cast<const float4*>(dup + ((n * Hp + yy) * (long long)Wp) * C) + c4;
      for (int v = vlo; v <= vhi; ++v) {
        const float wx = up_weight(sw, v, Ws, j);
        const int xx = v + pl;
        if (wx == 0.f || xx < 0 || xx >= Wp) continue;
        const float4 g = row[(long long)xx * C4];
        const float w = wy * wx;
        acc.x += w * g.x; acc.y += w * g.y; acc.z += w * g.z; acc.w += w * g.w;
      }
    }
    float4* o = reinterpret_cast<float4*>(dx) + e;
    if (accum) {
      const float4 a = *o;
      acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    *o = acc;
  }
}

// same adjoint with the destination windows precomputed (host-checked: each window spans <= 8 rows /
// columns, true for every x2-or-less upsample): the 8 row and 8 column weights (0 outside
// the window, the padded frame or the source support) are computed once per element instead of inside
// the 2-D loop, and only the nonzero taps issue loads
// (I: element index type, unsigned when N*Hs*Ws*C/4 < 2^31 — 32-bit divisions, as materialize_fast_kernel)
template <typename I = unsigned>
__global__ __launch_bounds__(256) void upsample_bwd4w_kernel(long long N, int C, int Hs, int Ws, int up_h, int up_w,
                                                             int pt, int pl, int Hp, int Wp, float sh, float sw,
                                                             const float* dup, float* dx, int accum) {
  const int C4 = C / 4;
  const I total = (I)(N * Hs * (long long)Ws * C4);
  for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (I)gridDim.x * blockDim.x) {
    I t = e / (I)C4;
    const int c4 = (int)(e - t * (I)C4);
    I t2 = t / (I)Ws;
    const int j = (int)(t - t2 * (I)Ws);
    t = t2 / (I)Hs;
    const int i = (int)(t2 - t * (I)Hs);
    const long long n = (long long)t;
    // u contributes to row i only if floor(sh*u) in {i-1, i}: u in [(i-1)/sh, (i+1)/sh] (+-1 guard)
    const int ulo = max(0, (int)ceilf((float)(i - 1) / sh) - 1), uhi = min(up_h - 1, (int)floorf((float)(i + 1) / sh) + 1);
    const int vlo = max(0, (int)ceilf((float)(j - 1) / sw) - 1), vhi = min(up_w - 1, (int)floorf((float)(j + 1) / sw) + 1);
    float wy[8], wx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int u = ulo + k, v = vlo + k;
      const int yy = u + pt, xx = v + pl;
      wy[k] = (u <= uhi && yy >= 0 && yy < Hp) ? up_weight(sh, u, Hs, i) : 0.f;
      wx[k] = (v <= vhi && xx >= 0 && xx < Wp) ? up_weight(sw, v, Ws, j) : 0.f;
    }
    // the 4 channels as two packed fp32 pairs (v_pk_fma_f32): the same fused multiply-add per channel
    typedef __attribute__((ext_vector_type(2))) float f2;
    f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 8; ++ky) {
      if (wy[ky] == 0.f) continue;
      const float4* row = reinterpret_cast<const float4*>(dup + ((n * Hp + ulo + ky + pt) * (long long)Wp) * C) + c4;
#pragma unroll
      for (int kx = 0; kx < 8; ++kx) {
        if (wx[kx] == 0.f) continue;
        const float4 g = row[(long long)(vlo + kx + pl) * C4];
        const float w = wy[ky] * wx[kx];
#if UNET_PK_UP
        const f2 ww = {w, w};
        a01 = __builtin_elementwise_fma(ww, f2{g.x, g.y}, a01);
        a23 = __builtin_elementwise_fma(ww, f2{g.z, g.w}, a23);
#else
        a01[0] += w * g.x; a01[1] += w * g.y; a23[0] += w * g.z; a23[1] += w * g.w;
#endif
      }
    }
    float4 acc = make_float4(a01[0], a01[1], a23[0], a23[1]);
    float4* o = reinterpret_cast<float4*>(dx) + e;
    if (accum) {
      const float4 a = *o;
      acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    *o = acc;
  }
}

// Tiled adjoint (round 5): a block owns one source row i of image n, UJ source columns and 64 channels.
//  phase 1 (vertical): t[v][c] = sum_u wy(u, i) d_up[u + pt][v + pl][c] for the tile's destination columns v, each
//    d_up vector loaded once per block (the block-uniform row window and weights: no per-element index math, no
//    divergent branches, ~11 independent 16-byte loads in flight per thread); t lands in LDS;
//  phase 2 (horizontal): dx[i][j][c] (+)= sum_v wx(v, j) t[v][c] from LDS, the column weights from a per-block
//    table of the window columns' (i0, lambda).
//  Logical blocks run (channel tile, column tile, row, image) fastest-first and are dealt contiguously per XCD
//    (xcd_block), so the d_up rows shared by source rows i and i + 1 are fetched into one XCD's L2 once; the
//    element-per-thread gather measured 1.44x its algorithmic HBM bytes.
//  Summation order: rows first, then columns (fixed: deterministic; fp32-rounding-level different from the
//  per-element kernel's w_y * w_x products).
constexpr int UPB_J = 16, UPB_CT = 16, UPB_VMAX = 56;
__global__ __launch_bounds__(256) void upsample_bwd_tile_kernel(int N, int C, int Hs, int Ws, int up_h, int up_w, int pt,
                                                                int pl, int Hp, int Wp, float sh, float sw,
                                                                const float* __restrict__ dup, float* dx, int accum,
                                                                int ntj, int ntc) {
  __shared__ float4 t[UPB_VMAX][UPB_CT];
  __shared__ int tab_i0[UPB_VMAX], tab_i1[UPB_VMAX];
  __shared__ float tab_l[UPB_VMAX];
  const int tid = threadIdx.x;
  const unsigned lb = xcd_block(blockIdx.x, gridDim.x);
  const int ct = (int)(lb % (unsigned)ntc);
  unsigned r = lb / (unsigned)ntc;
  const int jt = (int)(r % (unsigned)ntj);
  r /= (unsigned)ntj;
  const int i = (int)(r % (unsigned)Hs);
  const int n = (int)(r / (unsigned)Hs);
  const int C4 = C >> 2, c4 = ct * UPB_CT + (tid & (UPB_CT - 1));
  const int j0 = jt * UPB_J;
  // destination rows touching source row i (same window and +-1 guard as upsample_bwd4w; host-checked <= 8)
  const int ulo = max(0, (int)ceilf((float)(i - 1) / sh) - 1), uhi = min(up_h - 1, (int)floorf((float)(i + 1) / sh) + 1);
  float wy[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int u = ulo + k, yy = u + pt;
    wy[k] = (u <= uhi && yy >= 0 && yy < Hp) ? up_weight(sh, u, Hs, i) : 0.f;
  }
  // destination columns touching source columns [j0, j0 + UPB_J) (host-checked <= UPB_VMAX)
  const int jlast = min(Ws - 1, j0 + UPB_J - 1);
  const int vlo = max(0, (int)ceilf((float)(j0 - 1) / sw) - 1), vhi = min(up_w - 1, (int)floorf((float)(jlast + 1) / sw) + 1);
  const int nv = vhi - vlo + 1;
  if (tid < nv) {
    const int v = vlo + tid, xx = v + pl;
    int a0, a1;
    float l;
    lin_idx(sw, v, Ws, a0, a1, l);
    const bool ok = xx >= 0 && xx < Wp;
    tab_i0[tid] = ok ? a0 : -1;
    tab_i1[tid] = ok ? a1 : -1;
    tab_l[tid] = l;
  }
  // phase 1: one (column, channel vector) item per thread and trip
  const bool cok = c4 < C4;
  const size_t rowpix = (size_t)Wp * C4;
  const float4* base = reinterpret_cast<const float4*>(dup) + ((size_t)n * Hp + (ulo + pt)) * rowpix + c4;
  for (int it = tid >> 4; it < nv; it += 256 / UPB_CT) {
    const int xx = vlo + it + pl;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok && xx >= 0 && xx < Wp) {
      const float4* p = base + (size_t)xx * C4;
      float4 g[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = wy[k] != 0.f ? p[(size_t)k * rowpix] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        a.x = __builtin_fmaf(wy[k], g[k].x, a.x); a.y = __builtin_fmaf(wy[k], g[k].y, a.y);
        a.z = __builtin_fmaf(wy[k], g[k].z, a.z); a.w = __builtin_fmaf(wy[k], g[k].w, a.w);
      }
    }
    t[it][tid & (UPB_CT - 1)] = a;
  }
  __syncthreads();
  // phase 2: one (source column, channel vector) per thread
  const int j = j0 + (tid >> 4);
  if (j > jlast || !cok) return;
  const int vjlo = max(vlo, (int)ceilf((float)(j - 1) / sw) - 1), vjhi = min(vhi, (int)floorf((float)(j + 1) / sw) + 1);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int v = vjlo; v <= vjhi; ++v) {
    const int q = v - vlo;
    const float l = tab_l[q];
    const float w = (tab_i0[q] == j ? 1.f - l : 0.f) + (tab_i1[q] == j ? l : 0.f);
    const float4 g = t[q][tid & (UPB_CT - 1)];
    a.x = __builtin_fmaf(w, g.x, a.x); a.y = __builtin_fmaf(w, g.y, a.y);
    a.z = __builtin_fmaf(w, g.z, a.z); a.w = __builtin_fmaf(w, g.w, a.w);
  }
  float4* o = reinterpret_cast<float4*>(dx) + (((size_t)n * Hs + i) * Ws + j) * C4 + c4;
  if (accum) {
    const float4 b = *o;
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  *o = a;
}

// raw buffer loads (the 1x1 kernels' idiom, pw.hip): 16 bytes at vector + scalar byte offset, zeros past the buffer
constexpr unsigned UPB_OOB = 0x40000000u;   // >= every buffer size admitted by unet_upsample_bwd_pw_ok (< 1 GiB)
typedef __amdgpu_buffer_rsrc_t upb_rsrc_t;
__device__ __forceinline__ upb_rsrc_t upb_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 upb_ld(upb_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}

// The tiled adjoint with the attention gate's W_g input gradient (a 1x1 dgrad, Ci -> C channels, that used to
// read-modify-write d_up in a launch of its own) formed on the way in: phase 1 consumes
//   v = (sum over the Ci / 32 chunks in order of W_g^T . dgw) + d_up
// per destination pixel and channel, i.e. pw_conv_kernel's MFMA chain from a zero accumulator and its OMK == 1
// epilogue's one fp32 add, then the fmaf steps, LDS tile and phase 2 of upsample_bwd_tile_kernel: the result has the
// bits of the two launches, and d_up is read once instead of read, written and read.
//  A block owns R consecutive source rows, J source columns and 64 channels, and walks the union of its rows'
//  destination windows (2R + 2 live rows of a x2 map, where R one-row blocks walked 4R) once, in ascending order:
//    v formed once per destination pixel;  a[r] = fmaf(w(u, r), v, a[r]) for the (at most two) owned rows u feeds.
//  Each owned row's accumulator starts at +0 and takes its live destination rows in ascending order with the
//  weights of upsample_bwd_tile_kernel's wy[] expression.  A slot of weight 0 adds fmaf(0, x, a) = a there (a starts
//  as +0 and a fused multiply-add into +0 or a non-zero sum never yields -0), so leaving those slots out keeps every
//  bit: the chain of every (row, column, channel) is that kernel's.  Phase 2 is its phase 2, per owned row; neither J
//  nor R enters any sum.
//  A wave owns WA of the block's four 16-channel MFMA tiles, whose NCH weight fragments each (the packed transposed
//  weight, the A operand) stay in registers, and walks the window's destination columns 16 at a time: lane (i16, g)
//  holds column 16 grp + i16; its B operand is one 16-byte load of dgw channels 32 c + 8 g .. + 7 of that pixel, its
//  accumulator the float4 of channels 16 tile + 4 g .. + 3, the granularity of d_up's loads and of the LDS tile.
//  Row table: lane l of every wave evaluates destination row U0 + l of the window against the R owned rows; the
//  rows that feed an owned row are a ballot mask walked bit by bit, a row's weights read from its lane
//  (block-uniform scalars).  Rows of the last group past Hs have weight 0 everywhere and store nothing.
//  Loads: RB live rows are one stage; the next stage's loads are issued before the MFMAs and fmafs of the current
//  one.  Weight fragments, the column table and the row table are set up once per block.
//  OCC: waves per SIMD the register allocation is held to.
template <typename T, int NCH, int WA, int R, int J, int RB, int OCC>
__global__ __launch_bounds__(256, OCC) void upsample_bwd_pw_kernel(
    int N, int C, int Hs, int Ws, int up_h, int up_w, int pt, int pl, int Hp, int Wp, float sh, float sw,
    const float* __restrict__ dup, const uint4* __restrict__ dgw, const uint4* __restrict__ wt, float* dx, int accum,
    int ntj, int ntc) {
  typedef typename Mma<T>::frag F;
  __shared__ float4 t[R][UPB_VMAX][UPB_CT + 1];
  __shared__ int tab_i0[UPB_VMAX], tab_i1[UPB_VMAX];
  __shared__ float tab_l[UPB_VMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const unsigned lb = xcd_block(blockIdx.x, gridDim.x);
  const int ct = (int)(lb % (unsigned)ntc);
  unsigned rr = lb / (unsigned)ntc;
  const int jt = (int)(rr % (unsigned)ntj);
  rr /= (unsigned)ntj;
  const unsigned ngr = ((unsigned)Hs + R - 1) / R;
  const int ibase = (int)(rr % ngr) * R;
  const int n = (int)(rr / ngr);
  const int C4 = C >> 2;
  const int j0 = jt * J;
  const int jlast = min(Ws - 1, j0 + J - 1);
  const int vlo = max(0, (int)ceilf((float)(j0 - 1) / sw) - 1), vhi = min(up_w - 1, (int)floorf((float)(jlast + 1) / sw) + 1);
  const int nv = vhi - vlo + 1;   // (host-checked <= UPB_VMAX)
  if (tid < nv) {
    const int v = vlo + tid, xx = v + pl;
    int a0, a1;
    float l;
    lin_idx(sw, v, Ws, a0, a1, l);
    const bool ok = xx >= 0 && xx < Wp;
    tab_i0[tid] = ok ? a0 : -1;
    tab_i1[tid] = ok ? a1 : -1;
    tab_l[tid] = l;
  }
  // the row table (host-checked: the group's window spans <= 64 destination rows)
  const int U0 = max(0, (int)ceilf((float)(ibase - 1) / sh) - 1);
  float wr[R];
  bool feeds = false;
  {
    const int u = U0 + lane, yy = u + pt;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = ibase + r;
      const int ulo = max(0, (int)ceilf((float)(i - 1) / sh) - 1), uhi = min(up_h - 1, (int)floorf((float)(i + 1) / sh) + 1);
      wr[r] = (i < Hs && u >= ulo && u <= uhi && yy >= 0 && yy < Hp) ? up_weight(sh, u, Hs, i) : 0.f;
      feeds = feeds || wr[r] != 0.f;
    }
  }
  const unsigned long long live = __ballot(feeds);
  const int wa = wave % (4 / WA), wg = wave / (4 / WA);
  F wq[WA][NCH];
#pragma unroll
  for (int aa = 0; aa < WA; ++aa)
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      wq[aa][c] = __builtin_bit_cast(F, wt[((size_t)(ct * 4 + wa * WA + aa) * NCH + c) * 64 + lane]);
  const int cl = 4 * wa * WA + g;
  const size_t img = (size_t)Hp * Wp;
  const upb_rsrc_t dr = upb_rsrc(dup + (size_t)n * img * C, (unsigned)(img * C * 4));
  const upb_rsrc_t xr = upb_rsrc(dgw + (size_t)n * img * (4 * NCH), (unsigned)(img * (64 * NCH)));
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // phase 1: one column and WA channel vectors per lane; the wave's column groups in turn
  for (int it = 16 * wg + i16; it - i16 < nv; it += 16 * WA) {
    const int xx = vlo + it + pl;
    const bool ok = it < nv && xx >= 0 && xx < Wp;
    const unsigned dvo = ok ? (unsigned)xx * (unsigned)C * 4u + (unsigned)(ct * UPB_CT + cl) * 16u : UPB_OOB;
    const unsigned xvo = ok ? (unsigned)xx * (unsigned)(64 * NCH) + (unsigned)g * 16u : UPB_OOB;
    float4 a[R][WA];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int aa = 0; aa < WA; ++aa) a[r][aa] = z4;
    // a stage: RB live rows (slot < 0: none left, the loads read zeros and nothing is added)
    float4 dv[RB][WA], dvn[RB][WA];
    uint4 q[RB][NCH], qn[RB][NCH];
    int sl[RB], sln[RB];
    unsigned long long m = live;
#define UPB_STAGE_LOAD(DV, Q, SL)                                                                                   \
  _Pragma("unroll") for (int k = 0; k < RB; ++k) {                                                              \
    SL[k] = m ? (int)__builtin_ctzll(m) : -1;                                                                       \
    m &= m - 1ull;                                                                                                  \
    const unsigned row = SL[k] < 0 ? 0u : (unsigned)(U0 + SL[k] + pt) * (unsigned)Wp;                               \
    const unsigned dk = SL[k] < 0 ? UPB_OOB : dvo, xk = SL[k] < 0 ? UPB_OOB : xvo;                                  \
    _Pragma("unroll") for (int aa = 0; aa < WA; ++aa)                                                               \
        DV[k][aa] = __builtin_bit_cast(float4, upb_ld(dr, dk, row * (unsigned)C * 4u + (unsigned)aa * 64u));        \
    _Pragma("unroll") for (int c = 0; c < NCH; ++c)                                                                 \
        Q[k][c] = upb_ld(xr, xk, row * (unsigned)(64 * NCH) + (unsigned)c * 64u);                                   \
  }
    UPB_STAGE_LOAD(dv, q, sl)
    while (sl[0] >= 0) {
      UPB_STAGE_LOAD(dvn, qn, sln)
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        if (sl[k] < 0) continue;   // block-uniform
        f32x4 acc[WA];
#pragma unroll
        for (int aa = 0; aa < WA; ++aa) acc[aa] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int aa = 0; aa < WA; ++aa) acc[aa] = Mma<T>::mma(wq[aa][c], __builtin_bit_cast(F, q[k][c]), acc[aa]);
        float4 v[WA];
#pragma unroll
        for (int aa = 0; aa < WA; ++aa) {
          // pw_conv_kernel's accumulating fp32 epilogue: v = acc; v += old
          v[aa] = make_float4(acc[aa][0], acc[aa][1], acc[aa][2], acc[aa][3]);
          v[aa].x += dv[k][aa].x; v[aa].y += dv[k][aa].y; v[aa].z += dv[k][aa].z; v[aa].w += dv[k][aa].w;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wr[r]), sl[k]));
          if (w == 0.f) continue;   // block-uniform
#pragma unroll
          for (int aa = 0; aa < WA; ++aa) {
            a[r][aa].x = __builtin_fmaf(w, v[aa].x, a[r][aa].x); a[r][aa].y = __builtin_fmaf(w, v[aa].y, a[r][aa].y);
            a[r][aa].z = __builtin_fmaf(w, v[aa].z, a[r][aa].z); a[r][aa].w = __builtin_fmaf(w, v[aa].w, a[r][aa].w);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        sl[k] = sln[k];
#pragma unroll
        for (int aa = 0; aa < WA; ++aa) dv[k][aa] = dvn[k][aa];
#pragma unroll
        for (int c = 0; c < NCH; ++c) q[k][c] = qn[k][c];
      }
    }
#undef UPB_STAGE_LOAD
    if (it < nv) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int aa = 0; aa < WA; ++aa) t[r][it][cl + 4 * aa] = a[r][aa];
    }
  }
  __syncthreads();
  // phase 2: upsample_bwd_tile_kernel's, one (source column, channel vector) per thread and owned row
  const int cv = tid & (UPB_CT - 1), c4 = ct * UPB_CT + cv;
  for (int j = j0 + (tid >> 4); j <= jlast; j += 256 / UPB_CT) {
    const int vjlo = max(vlo, (int)ceilf((float)(j - 1) / sw) - 1), vjhi = min(vhi, (int)floorf((float)(j + 1) / sw) + 1);
    float4 a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = z4;
    for (int v = vjlo; v <= vjhi; ++v) {
      const int qi = v - vlo;
      const float l = tab_l[qi];
      const float w = (tab_i0[qi] == j ? 1.f - l : 0.f) + (tab_i1[qi] == j ? l : 0.f);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 gq = t[r][qi][cv];
        a[r].x = __builtin_fmaf(w, gq.x, a[r].x); a[r].y = __builtin_fmaf(w, gq.y, a[r].y);
        a[r].z = __builtin_fmaf(w, gq.z, a[r].z); a[r].w = __builtin_fmaf(w, gq.w, a[r].w);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ibase + r >= Hs) break;
      float4* o = reinterpret_cast<float4*>(dx) + (((size_t)n * Hs + ibase + r) * Ws + j) * C4 + c4;
      float4 s = a[r];
      if (accum) {
        const float4 b = *o;
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
      }
      *o = s;
    }
  }
}

// destination-column window of J source columns (upsample_bwd_tile_kernel's host check)
static int upb_vspan(int J, float sw) { return (int)floorf((float)(J + 1) / sw) + 4; }

template <typename T, int NCH, int WA, int R, int J, int RB, int OCC>
static void launch_upb_pw_tile(hipStream_t st, int N, int C, int Hs, int Ws, int up_h, int up_w, int pt, int pl, int Hp,
                               int Wp, float sh, float sw, const float* d_up, const void* dgw, const void* wt, float* dx,
                               int accum) {
  const int ntj = cdiv(Ws, J), ntc = C / 64;
  const unsigned nblk = (unsigned)((long long)N * cdiv(Hs, R) * ntj * ntc);
  hipLaunchKernelGGL((upsample_bwd_pw_kernel<T, NCH, WA, R, J, RB, OCC>), dim3(nblk), dim3(256), 0, st, N, C, Hs, Ws,
                     up_h, up_w, pt, pl, Hp, Wp, sh, sw, d_up, (const uint4*)dgw, (const uint4*)wt, dx, accum, ntj, ntc);
}

// The tile per chunk count NCH = Ci / 32, by measurement at the bench's four gate levels (4 images, bf16; us per call
// back to back, against the one-row tile this kernel replaced):
//   NCH 1 (C 64, 512^2)    2 tiles per wave, 2 rows, 24 columns, 2 rows per stage      142.4 -> 103.5
//   NCH 2 (C 128, 256^2)   4 tiles per wave, 4 rows, 24 columns, 1 row per stage        88.9 ->  58.5
//   NCH 4 (C 256, 128^2)   the same                                                     96.8 ->  42.0
//   NCH 8 (C 512, 64^2)    2 tiles per wave, 4 rows, 16 columns, 1 row per stage        81.4 ->  36.3
// With 4 tiles per wave a wave forms all 64 channels of its pixels and dgw is loaded by one wave, not by four: from
// NCH 2 on dgw is most of what a block loads.  24 source columns are 52 window columns, four 16-column groups for four
// waves (16 columns: 36, three groups).  4 rows hold 61 KB of LDS (two blocks per CU), which the 512^2 level does not
// repay.  Where the window of 24 columns does not fit the LDS tile (narrow maps) the same form runs on 16.
template <typename T>
static void launch_upb_pw(int nch, hipStream_t st, int N, int C, int Hs, int Ws, int up_h, int up_w, int pt, int pl,
                          int Hp, int Wp, float sh, float sw, const float* d_up, const void* dgw, const void* wt,
                          float* dx, int accum) {
#define UPB_ARGS st, N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, sh, sw, d_up, dgw, wt, dx, accum
  const bool j24 = upb_vspan(24, sw) <= UPB_VMAX;
  if (nch == 1) {
    if (j24) launch_upb_pw_tile<T, 1, 2, 2, 24, 2, 4>(UPB_ARGS);
    else launch_upb_pw_tile<T, 1, 2, 2, 16, 2, 4>(UPB_ARGS);
  } else if (nch == 2) {
    if (j24) launch_upb_pw_tile<T, 2, 4, 4, 24, 1, 2>(UPB_ARGS);
    else launch_upb_pw_tile<T, 2, 4, 4, 16, 1, 2>(UPB_ARGS);
  } else if (nch == 4) {
    if (j24) launch_upb_pw_tile<T, 4, 4, 4, 24, 1, 2>(UPB_ARGS);
    else launch_upb_pw_tile<T, 4, 4, 4, 16, 1, 2>(UPB_ARGS);
  } else {
    launch_upb_pw_tile<T, 8, 2, 4, 16, 1, 2>(UPB_ARGS);
  }
#undef UPB_ARGS
}

// NHWC gather adjoint: dx[n,i,j,c] (+)= Σ_{u,v} wy(u,i) wx(v,j) d_up[n, u+pt, v+pl, c]
__global__ void upsample_bwd_kernel(long long N, int C, int Hs, int Ws, int up_h, int up_w, int pt, int pl, int Hp,
                                    int Wp, float sh, float sw, const float* dup, float* dx, int accum) {
  const long long total = N * Hs * (long long)Ws * C;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c = e % C;
    long long t = e / C;
    const int j = t % Ws;
    t /= Ws;
    const int i = t % Hs;
    const long long n = t / Hs;
    int ulo, uhi, vlo, vhi;
    up_range(sh, i, Hs, up_h, ulo, uhi);
    up_range(sw, j, Ws, up_w, vlo, vhi);
    float acc = 0.f;
    for (int u = ulo; u <= uhi; ++u) {
      const float wy = up_weight(sh, u, Hs, i);
      if (wy == 0.f) continue;
      const int yy = u + pt;
      if (yy < 0 || yy >= Hp) continue;
      float racc = 0.f;
      for (int v = vlo; v <= vhi; ++v) {
        const float wx = up_weight(sw, v, Ws, j);
        if (wx == 0.f) continue;
        const int xx = v + pl;
        if (xx < 0 || xx >= Wp) continue;
        racc += wx * dup[((n * Hp + yy) * (long long)Wp + xx) * C + c];
      }
      acc += wy * racc;
    }
    dx[e] = accum ? dx[e] + acc : acc;
  }
}

// fp32 NCHW bilinear (align_corners=True) forward: y[nc, u, v]
__global__ void resize_nchw_kernel(long long NC, int Hi, int Wi, int Ho, int Wo, float sh, float sw, const float* x,
                                   float* y) {
  const long long total = NC * Ho * (long long)Wo;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int v = e % Wo;
    long long t = e / Wo;
    const int u = t % Ho;
    const long long nc = t / Ho;
    int y0, y1, x0, x1;
    float ly, lx;
    lin_idx(sh, u, Hi, y0, y1, ly);
    lin_idx(sw, v, Wi, x0, x1, lx);
    const float* p = x + nc * Hi * (long long)Wi;
    const float a = p[y0 * Wi + x0], b = p[y0 * Wi + x1], c = p[y1 * Wi + x0], d = p[y1 * Wi + x1];
    y[e] = (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
  }
}

__global__ void resize_nchw_bwd_kernel(long long NC, int Hi, int Wi, int Ho, int Wo, float sh, float sw, const float* dy,
                                       float* dx, int accum) {
  const long long total = NC * Hi * (long long)Wi;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int j = e % Wi;
    long long t = e / Wi;
    const int i = t % Hi;
    const long long nc = t / Hi;
    int ulo, uhi, vlo, vhi;
    up_range(sh, i, Hi, Ho, ulo, uhi);
    up_range(sw, j, Wi, Wo, vlo, vhi);
    const float* p = dy + nc * Ho * (long long)Wo;
    float acc = 0.f;
    for (int u = ulo; u <= uhi; ++u) {
      const float wy = up_weight(sh, u, Hi, i);
      if (wy == 0.f) continue;
      float racc = 0.f;
      for (int v = vlo; v <= vhi; ++v) {
        const float wx = up_weight(sw, v, Wi, j);
        if (wx != 0.f) racc += wx * p[u * (long long)Wo + v];
      }
      acc += wy * racc;
    }
    dx[e] = accum ? dx[e] + acc : acc;
  }
}

// I: upsample_bwd4w_kernel's element index type
template <typename I>
static int launch_upb4w(hipStream_t st, long long N, int C, int Hs, int Ws, int up_h, int up_w, int pt, int pl, int Hp,
                        int Wp, float sh, float sw, const float* d_up, float* dx, int accum) {
  const long long total4 = N * Hs * (long long)Ws * C / 4;
  hipLaunchKernelGGL(upsample_bwd4w_kernel<I>, dim3(grid_for(total4, block_cap("UNET_UPB_BLOCKS", 8192))), dim3(256), 0,
                     st, N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, sh, sw, d_up, dx, accum);
  return check_launch("upsample_bwd");
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_upsample_bwd(long long N, int C, int Hs, int Ws, int up_h, int up_w, int pad_t, int pad_l, int Hp, int Wp,
                      float sh, float sw, const float* d_up, float* dx, int accum, void* stream) {
  const long long total = N * Hs * (long long)Ws * C;
  hipStream_t st = (hipStream_t)stream;
  // widest destination window of upsample_bwd4w: floor(2/scale) + 3 taps (scale 0: the whole map)
  auto span = [](float sc, int up) { return sc > 0.f ? (int)floorf(2.f / sc) + 3 : up + 8; };
  if (C % 4 == 0 && span(sh, up_h) <= 8 && span(sw, up_w) <= 8) {
    // the tiled kernel: its destination-column window for UPB_J source columns must fit the LDS table
    const int vspan = (int)floorf((float)(UPB_J + 1) / sw) + 4;
    const char* e = getenv("UNET_UPB_TILE");
    const long long ntj = cdiv(Ws, UPB_J), ntc = cdiv(C / 4, UPB_CT), nblk = N * Hs * ntj * ntc;
    if (!(e && atoi(e) == 0) && vspan <= UPB_VMAX && nblk < (1LL << 31)) {
      hipLaunchKernelGGL(upsample_bwd_tile_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (int)N, C, Hs, Ws, up_h, up_w,
                         pad_t, pad_l, Hp, Wp, sh, sw, d_up, dx, accum, (int)ntj, (int)ntc);
      return check_launch("upsample_bwd");
    }
    if (total / 4 < (1LL << 31))
      return launch_upb4w<unsigned>(st, N, C, Hs, Ws, up_h, up_w, pad_t, pad_l, Hp, Wp, sh, sw, d_up, dx, accum);
    return launch_upb4w<unsigned long long>(st, N, C, Hs, Ws, up_h, up_w, pad_t, pad_l, Hp, Wp, sh, sw, d_up, dx, accum);
  }
  if (C % 4 == 0) {
    hipLaunchKernelGGL(upsample_bwd4_kernel, dim3(grid_for(total / 4, block_cap("UNET_UPB_BLOCKS", 8192))), dim3(256), 0,
                       st, N, C, Hs, Ws, up_h, up_w, pad_t, pad_l, Hp, Wp, sh, sw, d_up, dx, accum);
    return check_launch("upsample_bwd");
  }
  hipLaunchKernelGGL(upsample_bwd_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st, N, C, Hs, Ws, up_h, up_w, pad_t,
                     pad_l, Hp, Wp, sh, sw, d_up, dx, accum);
  return check_launch("upsample_bwd");
}

// geometry upsample_bwd_pw_kernel serves: the 16-bit operand types, whole 64-channel tiles, 1 / 2 / 4 / 8 chunks of
// 32 projection channels (the weight fragments are a register array), and the geometry on which unet_upsample_bwd
// launches upsample_bwd_tile_kernel (the fused result is defined as that kernel's chain).  A window is at most the
// whole map, so a map of up to 8 rows or columns is served whatever its scale (a 2-row source: scale 1/3, whose
// window bound rounds to 9); unet_upsample_bwd runs such a map on another kernel, and a caller that needs the bits
// of the two launches (AttentionGate.up_fused_ok) leaves those maps out.  The kernel's row table holds 64
// destination rows per row group: 19 at most at the scales admitted here
int unet_upsample_bwd_pw_ok(int dtype, long long N, int C, int Hs, int Ws, int up_h, int up_w, int pad_t, int pad_l,
                            int Hp, int Wp, float sh, float sw, int Ci) {
  if (dtype != UNET_BF16 && dtype != UNET_F16) return 0;
  if (N < 1 || C < 64 || C % 64 || (Ci != 32 && Ci != 64 && Ci != 128 && Ci != 256)) return 0;
  if (Hs < 1 || Ws < 1 || up_h < 1 || up_w < 1 || Hp < 1 || Wp < 1) return 0;
  auto span = [](float sc, int up) { return sc > 0.f ? min(up, (int)floorf(2.f / sc) + 3) : up + 8; };
  if (span(sh, up_h) > 8 || span(sw, up_w) > 8) return 0;
  const int vspan = (int)floorf((float)(UPB_J + 1) / sw) + 4;
  const char* e = getenv("UNET_UPB_TILE");
  const long long nblk = N * Hs * (long long)cdiv(Ws, UPB_J) * (C / 64);
  if ((e && atoi(e) == 0) || vspan > UPB_VMAX || nblk >= (1LL << 31) || N * Hs >= (1LL << 31)) return 0;
  // one image of d_up and of dgw is a raw buffer with 32-bit offsets
  const double img = (double)Hp * Wp;
  return img * C * 4 < (double)UPB_OOB && img * Ci * 2 < (double)UPB_OOB;
}

int unet_upsample_bwd_pw(int dtype, long long N, int C, int Hs, int Ws, int up_h, int up_w, int pad_t, int pad_l,
                         int Hp, int Wp, float sh, float sw, const float* d_up, const void* dgw, int Ci,
                         const void* wt_packed, float* dx, int accum, void* stream) {
  if (!unet_upsample_bwd_pw_ok(dtype, N, C, Hs, Ws, up_h, up_w, pad_t, pad_l, Hp, Wp, sh, sw, Ci)) {
    set_error("unet_upsample_bwd_pw: geometry not served (unet_upsample_bwd_pw_ok)");
    return -1;
  }
  UNET_DISPATCH_T16(dtype, launch_upb_pw<T>(Ci / 32, (hipStream_t)stream, (int)N, C, Hs, Ws, up_h, up_w, pad_t, pad_l, Hp,
                                            Wp, sh, sw, d_up, dgw, wt_packed, dx, accum));
  return check_launch("upsample_bwd_pw");
}

int unet_resize_nchw(long long NC, int Hi, int Wi, int Ho, int Wo, float sh, float sw, const float* x, float* y,
                     void* stream) {
  hipLaunchKernelGGL(resize_nchw_kernel, dim3(grid_for(NC * Ho * (long long)Wo, 8192)), dim3(256), 0,
                     (hipStream_t)stream, NC, Hi, Wi, Ho, Wo, sh, sw, x, y);
  return check_launch("resize_nchw");
}

int unet_resize_nchw_bwd(long long NC, int Hi, int Wi, int Ho, int Wo, float sh, float sw, const float* dy, float* dx,
                         int accum, void* stream) {
  hipLaunchKernelGGL(resize_nchw_bwd_kernel, dim3(grid_for(NC * Hi * (long long)Wi, 8192)), dim3(256), 0,
                     (hipStream_t)stream, NC, Hi, Wi, Ho, Wo, sh, sw, dy, dx, accum);
  return check_launch("resize_nchw_bwd");
}

}  // extern "C"
