// surface.hip — surface-distance metrics on the device: Hausdorff, its percentile (HD95) and ASSD per
// (image, class), DESIGN.md §14.
//
// For class c of image n, A = (P == c), B = (T == c); the surface S(A) is every pixel of A with a 4-neighbour
// outside A (the frame's outside is outside A): A ^ binary_erosion(A), the convention of medpy and MONAI.  The
// exact Euclidean distance of every surface pixel of one mask to the other mask's surface comes from a separable
// transform: a column pass (distance in rows to the nearest surface pixel of the column) and a row pass that takes
// min_x' wy*g(x')^2 + wx*(x-x')^2 only at the surface pixels of the source mask.  The order statistics come from a
// radix select over the bit patterns of the squared distances.  No floating-point atomics anywhere: two runs
// give the same bits.
#include "common.h"

namespace unet {

constexpr int SF_MAXK = 16;
constexpr int SF_MAXDIM = 2048;  // 2 * 2047^2 < 2^24: with unit spacing every squared distance is an exact fp32 integer
constexpr int SF_TX = 16;        // columns of an edge/column block
constexpr int SF_LW = SF_TX + 2; // its label tile with the one-pixel halo
constexpr int SF_SEG = 32;       // rows of a segment: one 32-bit surface mask per class
constexpr int SF_NONE = 255;     // label byte of "no class"
constexpr unsigned SF_FAR = 0xFFFFu;

// torch.argmax over the class planes, the rule of confusion_kernel (metrics.hip): first maximum wins, NaN is the max
__device__ __forceinline__ int sf_argmax(const float* zp, int C, long long HW) {
  float best = zp[0];
  int bi = 0;
  for (int k = 1; k < C; ++k) {
    const float v = zp[(long long)k * HW];
    if (!(best != best) && (v > best || v != v)) { best = v; bi = k; }
  }
  return bi;
}

// the surface rows of class k in rows [32 seg, 32 seg + 32) of column `col`, bit i = row 32 seg + i
template <int KP>
__device__ __forceinline__ void sf_masks(const unsigned char* surf, int seg, int col, int H, unsigned (&mk)[KP]) {
#pragma unroll
  for (int k = 0; k < KP; ++k) mk[k] = 0u;
  const int y0 = seg * SF_SEG, rows = min(SF_SEG, H - y0);
  for (int i = 0; i < rows; ++i) {
    const int s = surf[(y0 + i) * SF_TX + col];
#pragma unroll
    for (int k = 0; k < KP; ++k) mk[k] |= (unsigned)(s == k) << i;
  }
}

// ------------------------------------------------------------------------------------------------
// 1. edge and column pass.  Block = (map m, image n, 16 columns) over the whole height; thread = (column, row
// segment).  g[m][n][c][y][x] (uint16) = rows to the nearest surface pixel of class c in column x, 0xFFFF: none.
// LDS: label bytes with halo [(H+2)][18], surface bytes [H][16] (the class whose surface the pixel is on, else
// 255: a pixel has one label, so it is on one class's surface at most), and the last / first surface row of every
// (segment, class, column), turned in place into "last above the segment" / "first below it" by one scan.
// ------------------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void surface_edge_col_kernel(int N, int C, int K, int H, int W, const float* z,
                                                               const int64_t* plab, const int64_t* tlab,
                                                               uint16_t* g) {
  extern __shared__ unsigned char sf_lds[];
  const int nseg = (H + SF_SEG - 1) / SF_SEG;
  unsigned char* lab = sf_lds;
  unsigned char* surf = lab + (((size_t)(H + 2) * SF_LW + 3) & ~(size_t)3);
  int16_t* above = reinterpret_cast<int16_t*>(surf + (size_t)H * SF_TX);
  int16_t* below = above + (size_t)nseg * KP * SF_TX;
  const int x0 = blockIdx.x * SF_TX, n = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
  const long long HW = (long long)H * W;

  for (int i = tid; i < (H + 2) * SF_LW; i += 256) {
    const int y = i / SF_LW - 1, x = x0 + i % SF_LW - 1;
    int v = SF_NONE;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const long long px = (long long)y * W + x;
      long long l;
      if (m == 1) l = tlab[n * HW + px];
      else if (z) l = sf_argmax(z + (long long)n * C * HW + px, C, HW);
      else l = plab[n * HW + px];
      if (l >= 0 && l < K) v = (int)l;   // a label outside [0, K) belongs to no class
    }
    lab[i] = (unsigned char)v;
  }
  __syncthreads();
  for (int i = tid; i < H * SF_TX; i += 256) {
    const unsigned char* p = lab + ((i >> 4) + 1) * SF_LW + (i & 15) + 1;
    const int l = p[0];
    const bool s = l != SF_NONE && (p[-SF_LW] != l || p[SF_LW] != l || p[-1] != l || p[1] != l);
    surf[i] = (unsigned char)(s ? l : SF_NONE);
  }
  __syncthreads();

  const int col = tid & (SF_TX - 1);
  for (int seg = tid >> 4; seg < nseg; seg += 256 / SF_TX) {
    unsigned mk[KP];
    sf_masks<KP>(surf, seg, col, H, mk);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int idx = (seg * KP + k) * SF_TX + col;
      above[idx] = (int16_t)(mk[k] ? seg * SF_SEG + 31 - __clz(mk[k]) : -1);
      below[idx] = (int16_t)(mk[k] ? seg * SF_SEG + __ffs(mk[k]) - 1 : -1);
    }
  }
  __syncthreads();
  if (tid < KP * SF_TX) {   // thread = (class, column): the carried surface row across segments, both ways
    const int k = tid >> 4;
    int run = -1;
    for (int seg = 0; seg < nseg; ++seg) {
      const int idx = (seg * KP + k) * SF_TX + col, t = above[idx];
      above[idx] = (int16_t)run;
      if (t >= 0) run = t;
    }
    run = -1;
    for (int seg = nseg - 1; seg >= 0; --seg) {
      const int idx = (seg * KP + k) * SF_TX + col, t = below[idx];
      below[idx] = (int16_t)run;
      if (t >= 0) run = t;
    }
  }
  __syncthreads();

  if (x0 + col >= W) return;
  for (int seg = tid >> 4; seg < nseg; seg += 256 / SF_TX) {
    unsigned mk[KP];
    sf_masks<KP>(surf, seg, col, H, mk);
    const int y0 = seg * SF_SEG, rows = min(SF_SEG, H - y0);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < K) {
        const int idx = (seg * KP + k) * SF_TX + col, a = above[idx], b = below[idx];
        uint16_t* gp = g + ((((size_t)m * N + n) * K + k) * H + y0) * W + x0 + col;
        for (int i = 0; i < rows; ++i) {
          const unsigned lo = mk[k] & (0xFFFFFFFFu >> (31 - i)), hi = mk[k] >> i;   // rows <= y, rows >= y
          const int y = y0 + i;
          const int ya = lo ? y0 + 31 - __clz(lo) : a, yb = hi ? y + __ffs(hi) - 1 : b;
          unsigned d = SF_FAR;
          if (ya >= 0) d = (unsigned)(y - ya);
          if (yb >= 0) d = min(d, (unsigned)(yb - y));
          gp[(size_t)i * W] = (uint16_t)d;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// 2. row pass.  Block = 4 rows of one (direction, image, class), a wave per row.  dir 0: from the prediction's
// surface to the target's, dir 1 the other way.  The other mask's row of g, as wy * g^2 in fp32, sits in LDS; a
// lane on a surface pixel at x widens its window r = 1, 2, ... over x - r and x + r and stops when wx * r^2 >= best
// (every candidate further out is fl(wx r'^2 + row) >= fl(wx r^2)); the wave leaves when no lane is active.
// dist2[dir][n][c][y][x]: the squared distance, -1 off the surface; rows without a surface pixel are not written
// (rowcnt == 0 tells the select to skip them).  Per-row partials: count, max of d^2, sum of sqrt in fp64.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surface_row_kernel(int H, int W, const uint16_t* g, float wy, float wx,
                                                          float* dist2, unsigned* rowcnt, float* rowmax,
                                                          double* rowsum) {
  extern __shared__ float sf_row[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + wave, dir = blockIdx.z;
  const size_t NK = gridDim.y, nc = blockIdx.y, plane = (size_t)H * W;
  const bool live = y < H;
  const int yc = live ? y : H - 1;
  float* row = sf_row + (size_t)wave * W;
  const uint16_t* gs = g + ((size_t)dir * NK + nc) * plane + (size_t)yc * W;
  const uint16_t* go = g + ((size_t)(1 - dir) * NK + nc) * plane + (size_t)yc * W;
  float* d2 = dist2 + ((size_t)dir * NK + nc) * plane + (size_t)yc * W;

  bool any = false, other = false;
  if (live)
    for (int x = lane; x < W; x += 64) any |= gs[x] == 0;
  any = __ballot(any) != 0ull;
  if (any) {
    for (int x = lane; x < W; x += 64) {
      const unsigned v = go[x];
      row[x] = v == SF_FAR ? __builtin_inff() : wy * (float)(v * v);
      other |= v != SF_FAR;
    }
  }
  other = __ballot(other) != 0ull;   // false: the other surface is empty in the whole image (every column is FAR)
  __syncthreads();

  unsigned cnt = 0u;
  float mx = 0.f;
  double sum = 0.0;
  if (any) {
    for (int xb = 0; xb < W; xb += 64) {
      const int x = xb + lane;
      const bool inb = x < W, s = inb && gs[x] == 0;
      if (__ballot(s) == 0ull) {
        if (inb) d2[x] = -1.f;
        continue;
      }
      float best = s ? row[x] : 0.f;
      if (other) {
        for (int r = 1; r < W; ++r) {
          const float r2 = (float)(r * r);
          if (__ballot(s && wx * r2 < best) == 0ull) break;
          if (inb && x - r >= 0) best = fminf(best, fmaf(wx, r2, row[x - r]));
          if (x + r < W) best = fminf(best, fmaf(wx, r2, row[x + r]));
        }
      }
      if (inb) d2[x] = s ? best : -1.f;
      if (s) {
        ++cnt;
        mx = fmaxf(mx, best);
        sum += sqrt((double)best);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    sum += __shfl_xor(sum, o, 64);
  }
  if (live && lane == 0) {
    const size_t r = ((size_t)dir * NK + nc) * H + y;
    rowcnt[r] = cnt;
    rowmax[r] = mx;
    rowsum[r] = sum;
  }
}

// ------------------------------------------------------------------------------------------------
// 3. select.  Block = one (direction, image, class), 16 waves: the block's time is the latency of its passes over
// the dense dist2 plane, so it reads 16 bytes per lane where W allows and keeps many waves in flight.  Sums the row partials in a fixed order, then a 4-pass 8-bit
// radix select over the bit patterns of dist2 (non-negative floats order as unsigned integers; -1 has the sign bit)
// finds the element of rank k_lo = floor(q (m - 1)); one more pass finds the next larger element when the
// interpolation needs it and the run of equal values ends at k_lo.  sqrt is monotone, so selecting on d^2 and
// taking the root afterwards is the percentile of d.  dres[dir][nc] = {max d, percentile of d, sum d}, dcnt = m.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sf_member(unsigned bits, unsigned himask, unsigned prefix) {
  return !(bits & 0x80000000u) && (bits & himask) == prefix;
}

constexpr int SF_SEL_T = 1024;

// f(bits) for every element of the rows of `d` that hold a surface pixel; a wave per row, 16-byte loads if W % 4 == 0
template <typename F>
__device__ __forceinline__ void sf_scan_plane(const float* d, const unsigned* rc, int H, int W, int wave, int lane,
                                              F f) {
  for (int y = wave; y < H; y += SF_SEL_T / 64) {
    if (rc[y] == 0u) continue;
    const float* r = d + (size_t)y * W;
    if ((W & 3) == 0) {
#pragma unroll 2
      for (int x = lane; x < W / 4; x += 64) {
        const uint4 q = reinterpret_cast<const uint4*>(r)[x];
        f(q.x); f(q.y); f(q.z); f(q.w);
      }
    } else {
      for (int x = lane; x < W; x += 64) f(__float_as_uint(r[x]));
    }
  }
}

__global__ __launch_bounds__(SF_SEL_T) void surface_select_kernel(int H, int W, const float* dist2, const unsigned* rowcnt,
                                                             const float* rowmax, const double* rowsum, double qf,
                                                             double* dres, long long* dcnt) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wsum[4];
  __shared__ unsigned sel[3];
  __shared__ double rsum[256];
  __shared__ float rmax[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t idx = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const unsigned* rc = rowcnt + idx * H;
  const float* d = dist2 + idx * (size_t)H * W;

  {
    unsigned c = 0u;
    float mx = 0.f;
    double s = 0.0;
    if (tid < 256) {
      for (int y = tid; y < H; y += 256) {
        c += rc[y];
        mx = fmaxf(mx, rowmax[idx * H + y]);
        s += rowsum[idx * H + y];
      }
      hist[tid] = c;
      rmax[tid] = mx;
      rsum[tid] = s;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        hist[tid] += hist[tid + o];
        rmax[tid] = fmaxf(rmax[tid], rmax[tid + o]);
        rsum[tid] += rsum[tid + o];
      }
      __syncthreads();
    }
  }
  const unsigned m = hist[0];
  const double dmax = sqrt((double)rmax[0]), dsum = rsum[0];
  __syncthreads();
  if (m == 0u) {
    if (tid == 0) {
      dres[idx * 3 + 0] = 0.0;
      dres[idx * 3 + 1] = 0.0;
      dres[idx * 3 + 2] = 0.0;
      dcnt[idx] = 0;
    }
    return;
  }

  // numpy.percentile, linear: virtual index (m - 1) * (q / 100), its floor and the next rank
  const double pos = (double)(m - 1u) * qf;
  unsigned klo = (unsigned)floor(pos);
  double frac = pos - (double)klo;
  if (klo >= m - 1u) { klo = m - 1u; frac = 0.0; }

  unsigned prefix = 0u, k = klo, eq = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    sf_scan_plane(d, rc, H, W, wave, lane, [&](unsigned bits) {
      if (sf_member(bits, himask, prefix)) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
    });
    __syncthreads();
    const unsigned v = tid < 256 ? hist[tid] : 0u;   // the 256 bins sit in waves 0 to 3
    unsigned s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(s, o, 64);
      if (lane >= o) s += t;
    }
    if (lane == 63 && wave < 4) wsum[wave] = s;
    __syncthreads();
    unsigned incl = s;
    for (int w = 0; w < min(wave, 4); ++w) incl += wsum[w];
    const unsigned excl = incl - v;
    if (v && excl <= k && k < incl) {   // one bin holds rank k
      sel[0] = (unsigned)tid;
      sel[1] = excl;
      sel[2] = v;
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    k -= sel[1];
    eq = sel[2];
  }
  // prefix: the bits of rank k_lo; it is the k-th of eq equal elements
  unsigned hibits = prefix;
  if (frac > 0.0 && k + 1u >= eq) {   // rank k_lo + 1 is the smallest element above it
    unsigned mn = 0xFFFFFFFFu;
    sf_scan_plane(d, rc, H, W, wave, lane, [&](unsigned bits) {
      if (!(bits & 0x80000000u) && bits > prefix) mn = min(mn, bits);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, (unsigned)__shfl_xor(mn, o, 64));
    if (tid < 256) hist[tid] = 0xFFFFFFFFu;
    __syncthreads();
    if (lane == 0) hist[wave] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) hist[tid] = min(hist[tid], hist[tid + o]);
      __syncthreads();
    }
    hibits = hist[0];
  }
  if (tid == 0) {
    const double a = sqrt((double)__uint_as_float(prefix)), b = sqrt((double)__uint_as_float(hibits));
    const double diff = b - a;   // numpy's _lerp
    double p = frac >= 0.5 ? b - diff * (1.0 - frac) : a + diff * frac;
    if (diff == 0.0 || frac == 0.0) p = a;
    dres[idx * 3 + 0] = dmax;
    dres[idx * 3 + 1] = p;
    dres[idx * 3 + 2] = dsum;
    dcnt[idx] = (long long)m;
  }
}

// the two directions of every (image, class) into the [N, K] outputs; NaN where either surface is empty
__global__ void surface_combine_kernel(int NK, const double* dres, const long long* dcnt, double* hd, double* hdp,
                                       double* assd, int64_t* n_pred, int64_t* n_true) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NK) return;
  const double* a = dres + (size_t)i * 3;
  const double* b = dres + ((size_t)NK + i) * 3;
  const long long ca = dcnt[i], cb = dcnt[NK + i];
  const bool ok = ca > 0 && cb > 0;
  const double nan = __builtin_nan("");
  hd[i] = ok ? fmax(a[0], b[0]) : nan;
  hdp[i] = ok ? fmax(a[1], b[1]) : nan;
  assd[i] = ok ? (a[2] + b[2]) / (double)(ca + cb) : nan;
  n_pred[i] = ca;
  n_true[i] = cb;
}

struct SurfaceWs {
  size_t rowsum, dres, dcnt, dist2, rowmax, rowcnt, g, total;
};

static SurfaceWs surface_ws(long long N, int K, int H, int W) {
  const size_t NK = (size_t)N * K, rows = 2 * NK * H, px = rows * W;
  SurfaceWs w;
  size_t o = 0;
  w.rowsum = o; o += rows * sizeof(double);
  w.dres = o;   o += 2 * NK * 3 * sizeof(double);
  w.dcnt = o;   o += 2 * NK * sizeof(long long);
  w.dist2 = o;  o += px * sizeof(float);
  w.rowmax = o; o += rows * sizeof(float);
  w.rowcnt = o; o += rows * sizeof(unsigned);
  w.g = o;      o += px * sizeof(uint16_t);
  w.total = o;
  return w;
}

static bool surface_shape_ok(long long N, int K, int H, int W) {
  return N >= 1 && N <= 65535 && K >= 1 && K <= SF_MAXK && N * K <= 65535 && H >= 1 && H <= SF_MAXDIM && W >= 1 &&
         W <= SF_MAXDIM;
}

template <int KP>
static int surface_launch_edge(hipStream_t st, int N, int C, int K, int H, int W, const float* z, const int64_t* plab,
                               const int64_t* tlab, uint16_t* g) {
  const int nseg = (H + SF_SEG - 1) / SF_SEG;
  const size_t lds = (((size_t)(H + 2) * SF_LW + 3) & ~(size_t)3) + (size_t)H * SF_TX +
                     2 * (size_t)nseg * KP * SF_TX * sizeof(int16_t);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&surface_edge_col_kernel<KP>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("unet_surface_distances: cannot reserve the LDS tile"); return (int)e; }
  }
  hipLaunchKernelGGL((surface_edge_col_kernel<KP>), dim3(cdiv(W, SF_TX), N, 2), dim3(256), lds, st, N, C, K, H, W, z,
                     plab, tlab, g);
  return check_launch("surface_edge_col");
}

}  // namespace unet

using namespace unet;

extern "C" size_t unet_surface_workspace(long long N, int K, int H, int W) {
  return surface_shape_ok(N, K, H, W) ? surface_ws(N, K, H, W).total : 0;
}

extern "C" int unet_surface_distances(long long N, int C, int K, int H, int W, const float* logits,
                                      const int64_t* labels, const int64_t* targets, double sy, double sx,
                                      double quantile, void* workspace, double* hd, double* hd_percentile,
                                      double* assd, int64_t* n_pred, int64_t* n_true, void* stream) {
  if (!surface_shape_ok(N, K, H, W) || (logits && C < 1) || (!logits && !labels) || !targets || !workspace || !hd ||
      !hd_percentile || !assd || !n_pred || !n_true || !(sy > 0.0) || !(sx > 0.0) || !(sy < 1e15) || !(sx < 1e15) ||
      !(quantile >= 0.0 && quantile <= 1.0)) {
    set_error("unet_surface_distances: bad arguments (1 <= num_classes <= 16, 1 <= H, W <= 2048, N * K <= 65535, "
              "spacing > 0, 0 <= quantile <= 1)");
    return UNET_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const SurfaceWs w = surface_ws(N, K, H, W);
  char* base = (char*)workspace;
  uint16_t* g = (uint16_t*)(base + w.g);
  float* dist2 = (float*)(base + w.dist2);
  unsigned* rowcnt = (unsigned*)(base + w.rowcnt);
  float* rowmax = (float*)(base + w.rowmax);
  double* rowsum = (double*)(base + w.rowsum);
  double* dres = (double*)(base + w.dres);
  long long* dcnt = (long long*)(base + w.dcnt);
  const int NK = (int)(N * K);

  int rc = K <= 4   ? surface_launch_edge<4>(st, (int)N, C, K, H, W, logits, labels, targets, g)
           : K <= 8 ? surface_launch_edge<8>(st, (int)N, C, K, H, W, logits, labels, targets, g)
                    : surface_launch_edge<16>(st, (int)N, C, K, H, W, logits, labels, targets, g);
  if (rc) return rc;
  hipLaunchKernelGGL(surface_row_kernel, dim3(cdiv(H, 4), NK, 2), dim3(256), (size_t)4 * W * sizeof(float), st, H, W,
                     g, (float)(sy * sy), (float)(sx * sx), dist2, rowcnt, rowmax, rowsum);
  if ((rc = check_launch("surface_row"))) return rc;
  hipLaunchKernelGGL(surface_select_kernel, dim3(NK, 2), dim3(SF_SEL_T), 0, st, H, W, dist2, rowcnt, rowmax, rowsum,
                     quantile, dres, dcnt);
  if ((rc = check_launch("surface_select"))) return rc;
  hipLaunchKernelGGL(surface_combine_kernel, dim3(cdiv(NK, 256)), dim3(256), 0, st, NK, dres, dcnt, hd, hd_percentile,
                     assd, n_pred, n_true);
  return check_launch("surface_combine");
}
