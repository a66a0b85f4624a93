// stem.hip — the network's first convolution with 5 to 16 input channels (2.5-D CT stacks, multi-sequence MRI,
// multispectral bands): nn.Conv2d(n_channels -> 32 | 64, 3x3) reading the fp32 NCHW model input directly, forward
// and weight gradient on v_mfma_f32_16x16x32 for the 16-bit operand modes.  (Cin <= 4: smallcin.hip.)
//
// The input keeps the precision of the Cin <= 3 MFMA path: x = x_hi + x_lo, both 16-bit.  Here the split is done
// ONCE per staged element: the tile (8 rows x 64 columns + halo, [Cin][10][66]) lands in LDS as one dword
// {x_hi, x_lo} per element, filled by coalesced row loads of the NCHW planes.
//
// Forward: y[co][px] = Σ_k W[co][k] X[k][px], k = 2 (9 ci + tap) + half.  With `half` fastest, the two k of a
// dword are adjacent B-operand elements: a lane's 8 k of one K step are 4 LDS dwords, no conversion in the loop,
// and the A operand carries each weight twice.  The A fragments (up to 9 K steps x 4 channel fragments = 144
// VGPRs) live in LDS in fragment order, one 16-byte read per lane and fragment, shared by the 4 rows a wave
// accumulates per pass (4 rows x NF accumulators); the tap offsets of the runtime Cin come from a small LDS table.
// A wave owns 16 pixels of each tile row; epilogue and BN partial sums as smallcin_fwd_mfma_kernel.
//
// Weight gradient: D[co][k] = Σ_px dy[px][co] X[px][k], 32 pixels per MFMA.  The up to 18 sixteen-column
// fragments of k are dealt to the 4 waves (j = wave, wave + 4, ...: at most 5 each); every wave walks all pixels of
// the block's tiles.  The dy of one tile row (64 pixels) is staged once per block, double-buffered and prefetched a
// row ahead, in the swizzled layout ds_read_b64_tr_b16 turns into K-major fragments (wgrad5.hip); a lane's column k
// has a fixed half, so its B fragment is 8 LDS dwords and 4 v_perm.  Columns 2 jj and 2 jj + 1 (x_hi, x_lo) sit in
// neighbouring lanes and are added there; a block writes one slab [Cout][9 Cin] in dw's own order and
// slab_reduce_two_pass sums the slabs in a fixed order (no atomics: two runs give the same bits).
#include "conv_src16.h"
#include "paths.h"

namespace unet {

constexpr int ST_TR = 8, ST_TW = 64, ST_HW = ST_TW + 2, ST_PLANE = (ST_TR + 2) * ST_HW;
constexpr int ST_GRID = 512;   // persistent blocks (two per CU); forward stats rows = 4 per block
constexpr int ST_RP = 4;       // tile rows a wave accumulates per pass over the weight fragments
constexpr int ST_NI = 5;       // column fragments of k per wave in the weight gradient (18 over 4 waves)
constexpr int ST_RG = 32;      // scratch slabs of slab_reduce_two_pass (== pw.hip PW_RG)

static bool stem_on() {
  const char* e = getenv("UNET_STEM_MFMA");
  return !(e && !atoi(e));
}

// Cin = 4 is not here: tests/conv_cases.py pins it to the VALU kernel of smallcin.hip by name
bool stem_conv_ok(const unet_conv_desc* d) {
  return stem_on() && (d->dtype == UNET_BF16 || d->dtype == UNET_F16) && d->nsrc == 1 &&
         d->src[0].kind == UNET_SRC_NCHW_F32 && d->ksize == 3 && d->Cin >= 5 && d->Cin <= 16 &&
         (d->Cout == 32 || d->Cout == 64) && d->out_mode == UNET_OUT_Y && !d->bnb_y && !d->bnb_stats && !d->act_out &&
         (double)d->N * d->H * d->W < 2147483648.0;
}
bool stem_wgrad_ok(const unet_wgrad_desc* d) {
  return stem_on() && (d->dtype == UNET_BF16 || d->dtype == UNET_F16) && d->nsrc == 1 &&
         d->src[0].kind == UNET_SRC_NCHW_F32 && d->ksize == 3 && d->Cin >= 5 && d->Cin <= 16 &&
         (d->Cout == 32 || d->Cout == 64) && (double)d->N * d->H * d->W * d->Cout * 2 < (double)OOB;
}

// one element of the model input as the kernels hold it: {x_hi, x_lo} (x_hi = x rounded to T, x_lo = the rest)
template <typename T>
__device__ __forceinline__ unsigned stem_split(float v) {
  const T hi = (T)v;
  const T lo = (T)(v - (float)hi);
  return (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
}

// the input tile with halo of output rows h0.., columns w0..: xs[ci][row][col], zero outside the map
template <typename T>
__device__ __forceinline__ void stem_stage_x(unsigned* xs, const float* x, int n, int Cs, int Cin, int H, int W, int h0,
                                             int w0, int tid) {
  const int nel = Cin * ST_PLANE;
  for (int i = tid; i < nel; i += 256) {
    const int ci = i / ST_PLANE, rem = i - ci * ST_PLANE;
    const int rr = rem / ST_HW, cc = rem - rr * ST_HW;
    const int yy = h0 - 1 + rr, xx = w0 - 1 + cc;
    const float v = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                        ? x[(((size_t)n * Cs + ci) * H + yy) * W + xx] : 0.f;
    xs[i] = stem_split<T>(v);
  }
}

// LDS element of (ci, tap) = jj relative to an output pixel's own tile position; a padded jj reads the pixel's
// first tap (finite wherever the pixel's output is) against a zero weight, or into a column nobody stores
__device__ __forceinline__ int stem_tap_off(int jj, int K9) {
  const int ci = jj / 9, tap = jj - 9 * ci;
  return jj < K9 ? ci * ST_PLANE + (tap / 3) * ST_HW + tap % 3 : 0;
}

extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];

template <typename T, int COUT>
__global__ __launch_bounds__(256) void stem_fwd_mfma_kernel(const unet_conv_desc d, int ntiles) {
  using F = typename Mma<T>::frag;
  constexpr int NF = COUT / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int Cin = d.Cin, K9 = 9 * Cin, nks = (K9 + 15) / 16;
  uint4* wl = reinterpret_cast<uint4*>(st_smem);              // [nks][NF][64]: A fragments in lane order
  int* tab = reinterpret_cast<int*>(wl + nks * NF * 64);      // [16 nks]: tap offsets
  unsigned* xs = reinterpret_cast<unsigned*>(tab + 16 * nks); // [Cin][10][66]
  const int tiles_w = (d.W + ST_TW - 1) / ST_TW, tiles_h = (d.H + ST_TR - 1) / ST_TR;
  const float* x = (const float*)d.src[0].data;
  const int Cs = d.src[0].C;
  // A fragment (ks, f): lane (g, c16) holds W[co = 16 f + c16][jj = 16 ks + 4 g + p] twice (k = 2 jj, 2 jj + 1),
  // read from the packed forward weights (one chunk: Cin <= 32)
  {
    const unsigned short* wp = (const unsigned short*)d.weight;
    unsigned* wl32 = reinterpret_cast<unsigned*>(wl);
    for (int i = tid; i < nks * NF * 256; i += 256) {
      const int p = i & 3, ln = (i >> 2) & 63, ff = i >> 8;
      const int ks = ff / NF, f = ff - ks * NF;
      const int jj = 16 * ks + 4 * (ln >> 4) + p;
      unsigned w = 0;
      if (jj < K9) {
        const int ci = jj / 9, tap = jj - 9 * ci;
        w = wp[((size_t)(f * 9 + tap) * 64 + (ci >> 3) * 16 + (ln & 15)) * 8 + (ci & 7)];
      }
      wl32[i] = w | (w << 16);
    }
    for (int i = tid; i < 16 * nks; i += 256) tab[i] = stem_tap_off(i, K9);
  }
  float s1[NF][4], s2[NF][4];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[f][r] = 0.f; s2[f][r] = 0.f; }
  T* y = (T*)d.out;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tw = tile % tiles_w, t2 = tile / tiles_w;
    const int h0 = (t2 % tiles_h) * ST_TR, w0 = tw * ST_TW, n = t2 / tiles_h;
    __syncthreads();
    stem_stage_x<T>(xs, x, n, Cs, Cin, d.H, d.W, h0, w0, tid);
    __syncthreads();
    const int ow = w0 + 16 * wave + c16;
    for (int r0 = 0; r0 < ST_TR && h0 + r0 < d.H; r0 += ST_RP) {
      f32x4 acc[ST_RP][NF];
#pragma unroll
      for (int rr = 0; rr < ST_RP; ++rr)
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[rr][f] = f32x4{0.f, 0.f, 0.f, 0.f};
      const unsigned* xr = xs + r0 * ST_HW + 16 * wave + c16;
#pragma unroll 1
      for (int ks = 0; ks < nks; ++ks) {
        const int4 o = *reinterpret_cast<const int4*>(tab + 16 * ks + 4 * g);
        F a[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) a[f] = __builtin_bit_cast(F, wl[(ks * NF + f) * 64 + lane]);
#pragma unroll
        for (int rr = 0; rr < ST_RP; ++rr) {
          const unsigned* xq = xr + rr * ST_HW;
          const F b = __builtin_bit_cast(F, make_uint4(xq[o.x], xq[o.y], xq[o.z], xq[o.w]));
#pragma unroll
          for (int f = 0; f < NF; ++f) acc[rr][f] = Mma<T>::mma(a[f], b, acc[rr][f]);
        }
      }
      // lane (c16, g) holds channels 16 f + 4 g .. + 3 of pixel ow; the v_permlane16_swap re-pairing of
      // smallcin_fwd_mfma_kernel leaves row g with 8 contiguous channels: one 16-byte store per fragment pair
#pragma unroll
      for (int rr = 0; rr < ST_RP; ++rr) {
        if (h0 + r0 + rr < d.H) {   // block-uniform
          unsigned px_[NF], py_[NF];
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            px_[f] = pack2_16<T>(acc[rr][f][0], acc[rr][f][1]);
            py_[f] = pack2_16<T>(acc[rr][f][2], acc[rr][f][3]);
          }
          const size_t pix = ((size_t)n * d.H + h0 + r0 + rr) * d.W + ow;
#pragma unroll
          for (int f = 0; f < NF; f += 2) {
            const auto sx = __builtin_amdgcn_permlane16_swap(px_[f], px_[f + 1], false, false);
            const auto sy = __builtin_amdgcn_permlane16_swap(py_[f], py_[f + 1], false, false);
            if (ow < d.W)
              *reinterpret_cast<uint4*>(y + pix * COUT + 16 * (f + (g & 1)) + 8 * (g >> 1)) =
                  make_uint4(sx[0], sy[0], sx[1], sy[1]);
          }
          if (ow < d.W) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                s1[f][q] += acc[rr][f][q];
                s2[f][q] = __builtin_fmaf(acc[rr][f][q], acc[rr][f][q], s2[f][q]);
              }
          }
        }
      }
    }
  }
  if (!d.stats) return;
  const int rows = gridDim.x * 4, row = blockIdx.x * 4 + wave;
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float a1 = row16_sum(s1[f][q]), a2 = row16_sum(s2[f][q]);
      if (c16 == 0) {
        const int co = 16 * f + 4 * g + q;
        d.stats[(size_t)co * rows + row] = a1;
        d.stats[((size_t)COUT + co) * rows + row] = a2;
      }
    }
}

template <typename T, int COUT>
__global__ __launch_bounds__(256) void stem_wgrad_mfma_kernel(const unet_wgrad_desc d, int ntiles, float* part) {
  using F = typename Mma<T>::frag;
  constexpr int NF = COUT / 16, UPP = COUT / 8, PIXB = COUT * 2;   // 16-byte units / bytes of one dy pixel
  constexpr int UN = UPP / 4;                                      // units a thread stages per tile row
  constexpr int ROWB = ST_TW * PIXB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15, q = (lane >> 2) & 3, pp = lane & 3;
  const int Cin = d.Cin, K9 = 9 * Cin, K2 = 2 * K9;
  unsigned* xs = reinterpret_cast<unsigned*>(st_smem);            // [Cin][10][66]
  unsigned char* dyl = st_smem + (size_t)Cin * ST_PLANE * 4;      // [2][64 px][PIXB], swizzled
  const int tiles_w = (d.W + ST_TW - 1) / ST_TW, tiles_h = (d.H + ST_TR - 1) / ST_TR;
  const float* x = (const float*)d.src[0].data;
  const int Cs = d.src[0].C;
  const rsrc_t rdy = mk_rsrc(d.dy, (unsigned)((long long)d.N * d.H * d.W * PIXB));
  // B operand: this wave's column fragments j = wave + 4 i; the lane's column k = 16 j + c16 = 2 jj + half, so
  // half = c16 & 1 for every fragment: `sel` gathers that half of two neighbouring pixels' dwords
  int boff[ST_NI];
#pragma unroll
  for (int i = 0; i < ST_NI; ++i) {
    const int k = 16 * (wave + 4 * i) + c16;
    boff[i] = k < K2 ? stem_tap_off(k >> 1, K9) : 0;
  }
  const unsigned sel = (c16 & 1) ? 0x07060302u : 0x05040100u;
  // A operand (dy, 16 co x 32 px): pixel px of the staged row = UPP units of 8 channels, unit u stored at
  // u ^ swz(px) (UPP = 8: wgrad5's permutation, conflict-free transposed reads; UPP = 4: its low bit pair)
  auto swz = [](int px) { return UPP == 8 ? 2 * ((px >> 1) & 1) + 4 * ((px >> 3) & 1) : 2 * ((px >> 1) & 1); };
  unsigned aoff[2][NF];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int px = 8 * g + 4 * h + q, u = 2 * f + (pp >> 1);
      aoff[h][f] = (unsigned)(px * PIXB + ((u ^ swz(px)) * 16) + 8 * (pp & 1));
    }
  unsigned woff[UN], goff[UN];   // this thread's staged units: LDS byte offset, and (pixel, byte) in the dy row
  int gpx[UN];
#pragma unroll
  for (int k = 0; k < UN; ++k) {
    const int i = tid + 256 * k, px = i / UPP, u = i % UPP;
    woff[k] = (unsigned)(px * PIXB + ((u ^ swz(px)) * 16));
    gpx[k] = px;
    goff[k] = (unsigned)u * 16u;
  }
  f32x4 acc[ST_NI][NF];
#pragma unroll
  for (int i = 0; i < ST_NI; ++i)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tw = tile % tiles_w, t2 = tile / tiles_w;
    const int h0 = (t2 % tiles_h) * ST_TR, w0 = tw * ST_TW, n = t2 / tiles_h;
    const int nr = d.H - h0 < ST_TR ? d.H - h0 : ST_TR;
    uint4 nx[UN];
    auto load_dy = [&](int r) {
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        const int ow = w0 + gpx[k];
        const unsigned pix = ((unsigned)n * d.H + h0 + r) * (unsigned)d.W + ow;
        nx[k] = bld(rdy, ow < d.W ? pix * (unsigned)PIXB + goff[k] : OOB, 0);
      }
    };
    load_dy(0);
    __syncthreads();   // every wave has left the previous tile
    stem_stage_x<T>(xs, x, n, Cs, Cin, d.H, d.W, h0, w0, tid);
#pragma unroll 1
    for (int r = 0; r < nr; ++r) {
      // row r's dy into buffer r & 1 (its readers of row r - 2 are behind the barrier of row r - 1)
      unsigned char* buf = dyl + (r & 1) * ROWB;
#pragma unroll
      for (int k = 0; k < UN; ++k) *reinterpret_cast<uint4*>(buf + woff[k]) = nx[k];
      if (r + 1 < nr) load_dy(r + 1);
      __syncthreads();
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {   // the row's two 32-pixel K steps
        F a[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const unsigned char* b0 = buf + hh * 32 * PIXB;
          const i16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(b0 + aoff[0][f]));
          const i16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(b0 + aoff[1][f]));
          a[f] = __builtin_bit_cast(F, __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7));
        }
        const unsigned* xr = xs + r * ST_HW + 32 * hh + 8 * g;
#pragma unroll
        for (int i = 0; i < ST_NI; ++i) {
          if (16 * (wave + 4 * i) < K2) {   // wave-uniform
            const unsigned* xq = xr + boff[i];
            const F b = __builtin_bit_cast(F, make_uint4(__builtin_amdgcn_perm(xq[1], xq[0], sel),
                                                         __builtin_amdgcn_perm(xq[3], xq[2], sel),
                                                         __builtin_amdgcn_perm(xq[5], xq[4], sel),
                                                         __builtin_amdgcn_perm(xq[7], xq[6], sel)));
#pragma unroll
            for (int f = 0; f < NF; ++f) acc[i][f] = Mma<T>::mma(a[f], b, acc[i][f]);
          }
        }
      }
    }
  }
  // the block's slab [COUT][9 Cin]: lane (g, c16) holds D[co = 16 f + 4 g + r][k = 16 j + c16]; the x_hi and
  // x_lo columns of one (ci, tap) are lanes c16, c16 ^ 1
  float* pr = part + (size_t)blockIdx.x * COUT * K9;
#pragma unroll
  for (int i = 0; i < ST_NI; ++i) {
    const int k = 16 * (wave + 4 * i) + c16;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[i][f][r] + __shfl_xor(acc[i][f][r], 1, 64);
        if (!(c16 & 1) && k < K2) pr[(16 * f + 4 * g + r) * K9 + (k >> 1)] = v;
      }
  }
}

// ---- host ---------------------------------------------------------------------------------------------
static int stem_tiles(int N, int H, int W) { return N * cdiv(H, ST_TR) * cdiv(W, ST_TW); }
static int stem_grid(int tiles) { return tiles < ST_GRID ? tiles : ST_GRID; }

int stem_stats_rows(const unet_conv_desc* d) { return 4 * stem_grid(stem_tiles(d->N, d->H, d->W)); }

// the partial slabs, one per block, and slab_reduce_two_pass's scratch slabs
size_t stem_wgrad_ws(const unet_wgrad_desc* d) {
  return (size_t)(stem_grid(stem_tiles(d->N, d->H, d->W)) + ST_RG) * d->Cout * 9 * d->Cin * sizeof(float);
}

template <typename K>
static int stem_reserve_lds(K kernel, size_t lds) {
  if (lds <= 64 * 1024) return 0;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { set_error("stem: cannot reserve the LDS tile"); return (int)e; }
  return 0;
}

template <typename T, int COUT>
static int launch_stem_fwd(const unet_conv_desc* d, hipStream_t st) {
  const int t = stem_tiles(d->N, d->H, d->W), nks = cdiv(9 * d->Cin, 16);
  const size_t lds = (size_t)nks * (COUT / 16) * 1024 + (size_t)nks * 64 + (size_t)d->Cin * ST_PLANE * 4;
  if (const int e = stem_reserve_lds(&stem_fwd_mfma_kernel<T, COUT>, lds)) return e;
  hipLaunchKernelGGL((stem_fwd_mfma_kernel<T, COUT>), dim3(stem_grid(t)), dim3(256), lds, st, *d, t);
  return check_launch("stem_fwd_mfma");
}

int stem_conv(const unet_conv_desc* d, hipStream_t st) {
  if (d->Cout == 64) return UNET_DISPATCH_T16(d->dtype, launch_stem_fwd<T, 64>(d, st));
  return UNET_DISPATCH_T16(d->dtype, launch_stem_fwd<T, 32>(d, st));
}

template <typename T, int COUT>
static int launch_stem_wgrad(const unet_wgrad_desc* d, int grid, int tiles, hipStream_t st) {
  const size_t lds = (size_t)d->Cin * ST_PLANE * 4 + 2 * ST_TW * COUT * 2;
  if (const int e = stem_reserve_lds(&stem_wgrad_mfma_kernel<T, COUT>, lds)) return e;
  hipLaunchKernelGGL((stem_wgrad_mfma_kernel<T, COUT>), dim3(grid), dim3(256), lds, st, *d, tiles,
                     (float*)d->workspace);
  return check_launch("stem_wgrad_mfma");
}

int stem_wgrad(const unet_wgrad_desc* d, hipStream_t st) {
  const int t = stem_tiles(d->N, d->H, d->W), grid = stem_grid(t);
  const int e = d->Cout == 64 ? UNET_DISPATCH_T16(d->dtype, launch_stem_wgrad<T, 64>(d, grid, t, st))
                              : UNET_DISPATCH_T16(d->dtype, launch_stem_wgrad<T, 32>(d, grid, t, st));
  if (e) return e;
  const long long total = (long long)d->Cout * 9 * d->Cin;
  float* part = (float*)d->workspace;
  return slab_reduce_two_pass(part, grid, total, part + (size_t)grid * total, d->dw, d->accum, st);
}

}  // namespace unet
