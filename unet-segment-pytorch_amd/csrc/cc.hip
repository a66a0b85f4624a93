// cc.hip — connected components of a label map on the device: labelling, areas, counts and the size / largest
// filter, DESIGN.md §15.
//
// A component is a maximal set of pixels of one class joined through 4- or 8-neighbourhoods; its id is the smallest
// linear index y * W + x of its pixels, so every output is a function of the input alone.  Union-find by smaller
// index: a parent is always smaller than its child, a link is one atomicMin, nobody waits for anybody.
//   1. tile    one workgroup per 64 x 64 tile: runs by ballot, vertical / diagonal links on an LDS parent table,
//              roots and per-root pixel counts out to the global parent array and `area`
//   2. seam    one thread per pixel next to a tile border: the same union on the global parent array
//   3. flatten every pixel finds its root (comp); tile-local counts are added at the root; roots are counted
//   4. filter  [select the largest per (image, class),] apply min_size / keep_largest
// Integer atomics only: two runs give the same bits.
#include "common.h"

namespace unet {

constexpr int CC_MAXK = 16;
constexpr int CC_MAXDIM = 4096;
constexpr int CC_T = 64;          // tile edge: a wave is a tile row
constexpr int CC_LW = CC_T + 2;   // a row of class bytes with its border
constexpr int CC_NONE = 255;      // class byte of "no class"; in the link tables also background: links nothing
constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP, DEV = __HIP_MEMORY_SCOPE_AGENT;

// torch.argmax over the class planes, the rule of confusion_kernel (metrics.hip) and sf_argmax (surface.hip):
// first maximum wins, NaN is the max
__device__ __forceinline__ int cc_argmax(const float* zp, int C, long long HW) {
  float best = zp[0];
  int bi = 0;
  for (int k = 1; k < C; ++k) {
    const float v = zp[(long long)k * HW];
    if (!(best != best) && (v > best || v != v)) { best = v; bi = k; }
  }
  return bi;
}

// Root of x.  par[x] <= x everywhere and only ever decreases, so the walk ends, whatever other threads do meanwhile.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* par, int x) {
  int p;
  while ((p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, SCOPE)) != x) x = p;
  return x;
}

// Join the sets of a and b under the smaller root.  atomicMin(par[a], b) with b < a either finds a a root (done) or
// returns its former parent `old` < a, which still has to meet b: go on with (old, b).  max(a, b) falls in every
// round, so the loop ends; it never waits for another thread's store.
template <int SCOPE>
__device__ __forceinline__ void cc_union(int* par, int a, int b) {
  a = cc_find<SCOPE>(par, a);
  b = cc_find<SCOPE>(par, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) break;
    a = old;
  }
}

// ------------------------------------------------------------------------------------------------
// 1. tile pass.  Block = one 64 x 64 tile of one image, thread = (row wave + 4k, column lane).  LDS: class bytes
// [66][66] with a border of CC_NONE (pixels of other tiles are the seam pass's), the parent table and a count table,
// int32 per tile pixel.  A row's runs come from two ballots (run starts, run ends); par = the run's first pixel, cnt =
// the run's length there.  A run is linked to the row above only at the first column of each overlap: a pixel with
// the class above it links unless its left neighbour and that one's upper neighbour continue both runs; for
// connectivity 8 a pixel without its class above links to the upper-left / upper-right pixel unless its left / right
// neighbour lies under that pixel.  Roots stay in registers; a run start that is no root adds its length at the root.
// Out: cls; parent = image-linear index of the tile-local root, -1 for unlabelled pixels; area = the tile-local
// count at a tile-local root, 0 elsewhere.  The blocks of tile 0 clear their image's row of `count`.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_tile_kernel(int C, int K, int H, int W, int tiles_x, int tiles_y,
                                                      const float* z, const int64_t* labels, const uint8_t* mask,
                                                      int conn8, int background, uint8_t* cls, int* parent,
                                                      int* area, unsigned long long* count) {
  __shared__ unsigned char lab[CC_LW * CC_LW];
  __shared__ int par[CC_T * CC_T];
  __shared__ int cnt[CC_T * CC_T];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tpi = tiles_x * tiles_y;
  const int n = (int)(blockIdx.x / (unsigned)tpi), t = (int)(blockIdx.x - (unsigned)n * tpi);
  const int y0 = t / tiles_x * CC_T, x0 = t % tiles_x * CC_T;
  const long long HW = (long long)H * W, img = n * HW;
  if (t == 0 && tid < K) count[(long long)n * K + tid] = 0ull;

  for (int i = tid; i < CC_LW * CC_LW; i += 256) {
    const int r = i / CC_LW - 1, c = i % CC_LW - 1, y = y0 + r, x = x0 + c;
    int v = CC_NONE;
    if (r >= 0 && r < CC_T && c >= 0 && c < CC_T && y < H && x < W) {
      const long long px = (long long)y * W + x;
      long long l;
      if (z) l = cc_argmax(z + (long long)n * C * HW + px, C, HW);
      else if (labels) l = labels[img + px];
      else l = mask[img + px] > 127;
      if (l >= 0 && l < K) v = (int)l;   // a label outside [0, K) belongs to no class
      cls[img + px] = (uint8_t)v;
      if (v == background) v = CC_NONE;
    }
    lab[i] = (unsigned char)v;
  }
  __syncthreads();

  for (int r = wave; r < CC_T; r += 4) {
    const unsigned char* p = lab + (r + 1) * CC_LW + lane + 1;
    const int v = p[0];
    const bool act = v != CC_NONE;
    const unsigned long long starts = __ballot(act && p[-1] != v), ends = __ballot(act && p[1] != v);
    int pr = -1, len = 0;
    if (act) {   // the border makes a start at or below and an end at or above every labelled lane
      const int s = 63 - __clzll((long long)(starts & ((2ull << lane) - 1ull)));
      pr = r * CC_T + s;
      if (s == lane) len = __ffsll((unsigned long long)(ends >> lane));
    }
    par[r * CC_T + lane] = pr;
    cnt[r * CC_T + lane] = len;
  }
  __syncthreads();

  for (int r = wave; r < CC_T; r += 4) {
    const unsigned char* p = lab + (r + 1) * CC_LW + lane + 1;
    const unsigned char* u = p - CC_LW;
    const int v = p[0], i = r * CC_T + lane;
    if (v == CC_NONE) continue;
    if (u[0] == v) {
      if (!(p[-1] == v && u[-1] == v)) cc_union<WG>(par, i, i - CC_T);
    } else if (conn8) {
      if (u[-1] == v && p[-1] != v) cc_union<WG>(par, i, i - CC_T - 1);
      if (u[1] == v && p[1] != v) cc_union<WG>(par, i, i - CC_T + 1);
    }
  }
  __syncthreads();

  int root[CC_T / 4];
#pragma unroll
  for (int k = 0; k < CC_T / 4; ++k) {
    const int i = (wave + 4 * k) * CC_T + lane;
    root[k] = par[i] >= 0 ? cc_find<WG>(par, i) : -1;
  }
#pragma unroll
  for (int k = 0; k < CC_T / 4; ++k) {   // cnt[i] of a pixel that is no root is its own thread's alone
    const int i = (wave + 4 * k) * CC_T + lane;
    if (root[k] >= 0 && root[k] != i && cnt[i] > 0) atomicAdd(&cnt[root[k]], cnt[i]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_T / 4; ++k) {
    const int r = wave + 4 * k, i = r * CC_T + lane, y = y0 + r, x = x0 + lane;
    if (y < H && x < W) {
      const long long px = img + (long long)y * W + x;
      parent[px] = root[k] < 0 ? -1 : (y0 + (root[k] >> 6)) * W + x0 + (root[k] & 63);
      area[px] = root[k] == i ? cnt[i] : 0;
    }
  }
}

// the link class of pixel (y, x) of one image: CC_NONE outside the frame, for no class and for background
__device__ __forceinline__ int cc_link_class(const uint8_t* cls, int H, int W, int y, int x, int background) {
  if (y < 0 || y >= H || x < 0 || x >= W) return CC_NONE;
  const int v = cls[(long long)y * W + x];
  return v == background ? CC_NONE : v;
}

// ------------------------------------------------------------------------------------------------
// 2. seam pass.  Thread = one pixel q on the far side of a tile border: column x = 64 j of a vertical border (its
// partners are in column x - 1), or row y = 64 j of a horizontal one (partners in row y - 1).  With `along` the
// direction of the border and b the pixel across it, the rule of the tile pass holds turned by 90 degrees: q links
// to b unless the previous pixel along the border and its partner continue both sides; without b in its class, q
// links to the partner before / after b unless q's own neighbour along the border lies next to that partner.  The
// pixels this rule leans on are joined inside a tile or by another thread of this launch, in whatever order; where
// the previous pixel along the border lies in another tile (a tile corner) q always links to b, or the two borders
// that meet there would each leave the link to the other.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_seam_kernel(long long total, int H, int W, int nvx, int nhy, int conn8,
                                                      int background, const uint8_t* cls, int* parent) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int per = nvx * H + nhy * W, nv = nvx * H;
  const long long n = g / per;
  int it = (int)(g - n * per), y, x, ay, ax, by, bx;
  if (it < nv) {
    x = (it / H + 1) * CC_T; y = it % H; ay = 1; ax = 0; by = y; bx = x - 1;
  } else {
    it -= nv;
    y = (it / W + 1) * CC_T; x = it % W; ay = 0; ax = 1; by = y - 1; bx = x;
  }
  cls += n * H * W;
  parent += n * H * W;
  const int v = cc_link_class(cls, H, W, y, x, background);
  if (v == CC_NONE) return;
  const int q = y * W + x;
  if (cc_link_class(cls, H, W, by, bx, background) == v) {
    if (((ay ? y : x) & (CC_T - 1)) == 0 || !(cc_link_class(cls, H, W, y - ay, x - ax, background) == v &&
          cc_link_class(cls, H, W, by - ay, bx - ax, background) == v))
      cc_union<DEV>(parent, q, by * W + bx);
  } else if (conn8) {
    if (cc_link_class(cls, H, W, by - ay, bx - ax, background) == v &&
        cc_link_class(cls, H, W, y - ay, x - ax, background) != v)
      cc_union<DEV>(parent, q, (by - ay) * W + bx - ax);
    if (cc_link_class(cls, H, W, by + ay, bx + ax, background) == v &&
        cc_link_class(cls, H, W, y + ay, x + ax, background) != v)
      cc_union<DEV>(parent, q, (by + ay) * W + bx + ax);
  }
}

// ------------------------------------------------------------------------------------------------
// 3. flatten.  Thread = pixel.  comp = the root; a tile-local root (area > 0) that is not the component's root moves
// its count to the root: area of such a pixel is touched by its own thread alone, the root's only by atomic adds.
// Every root adds one to count[n][class].
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_flatten_kernel(long long total, unsigned HW, int K, const int* parent,
                                                         const uint8_t* cls, int* comp, int* area,
                                                         unsigned long long* count) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  int r = parent[g];
  if (r < 0) { comp[g] = -1; return; }
  const unsigned n = (unsigned)g / HW;
  const long long base = (long long)n * HW;
  for (int p; (p = parent[base + r]) != r;) r = p;
  comp[g] = r;
  if (base + r != g) {
    const int a = area[g];
    if (a > 0) { atomicAdd(&area[base + r], a); area[g] = 0; }
  } else {
    atomicAdd(&count[(long long)n * K + cls[g]], 1ull);
  }
}

// ------------------------------------------------------------------------------------------------
// 4. filter.  best[n][c] = max over the roots of (area << 32) | (0x7fffffff - id): the largest area, the smaller id
// on a tie.  The apply kernel writes V pixels per thread in one store of up to 16 bytes.
// ------------------------------------------------------------------------------------------------
__global__ void cc_clear_kernel(long long n, unsigned long long* best) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) best[i] = 0ull;
}

__global__ __launch_bounds__(256) void cc_select_kernel(long long total, unsigned HW, int K, const int* comp,
                                                        const int* area, const uint8_t* cls,
                                                        unsigned long long* best) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const unsigned n = (unsigned)g / HW;
  const int q = (int)((unsigned)g - n * HW);
  if (comp[g] != q) return;
  atomicMax(&best[(long long)n * K + cls[g]],
            ((unsigned long long)(unsigned)area[g] << 32) | (unsigned long long)(0x7fffffffu - (unsigned)q));
}

template <int V, typename OUT>
__global__ __launch_bounds__(256) void cc_apply_kernel(long long total, unsigned HW, int K, const int* comp,
                                                       const int* area, const uint8_t* cls, long long min_size,
                                                       int background, long long fill,
                                                       const unsigned long long* best, OUT* out) {
  const long long g0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (g0 >= total) return;   // total is a multiple of V
  constexpr int AL = V * sizeof(OUT) < 16 ? V * sizeof(OUT) : 16;
  int cp[V];
  unsigned char cl[V];
  OUT res[V];
  __builtin_memcpy(cp, __builtin_assume_aligned(comp + g0, V * 4 < 16 ? V * 4 : 16), sizeof(cp));
  __builtin_memcpy(cl, __builtin_assume_aligned(cls + g0, V < 16 ? V : 16), sizeof(cl));
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int r = cp[j], c = cl[j];
    bool keep = false;
    if (r >= 0) {
      const unsigned n = (unsigned)(g0 + j) / HW;
      keep = (long long)area[(long long)n * HW + r] >= min_size;
      if (keep && best) keep = (int)(0x7fffffffu - (unsigned)best[(long long)n * K + c]) == r;
    }
    if constexpr (sizeof(OUT) == 1) res[j] = (OUT)(keep && c == 1 ? 255 : 0);
    else res[j] = (OUT)(keep || (r < 0 && c == background) ? c : fill);
  }
  __builtin_memcpy(__builtin_assume_aligned(out + g0, AL), res, sizeof(res));
}

static bool cc_shape_ok(long long N, int H, int W) {
  return N >= 1 && H >= 1 && H <= CC_MAXDIM && W >= 1 && W <= CC_MAXDIM && N * H * W < (1ll << 31);
}

// workspace: best [N][16] (uint64), then parent [N][H][W] (int32)
static size_t cc_best_bytes(long long N) { return (size_t)N * CC_MAXK * sizeof(unsigned long long); }

static bool cc_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <typename OUT>
static int cc_launch_apply(hipStream_t st, long long total, unsigned HW, int K, const int* comp, const int* area,
                           const uint8_t* cls, long long min_size, int background, long long fill,
                           const unsigned long long* best, OUT* out) {
  constexpr int V = 16 / sizeof(OUT);
  if (total % V == 0 && cc_aligned16(comp) && cc_aligned16(cls) && cc_aligned16(out))
    hipLaunchKernelGGL((cc_apply_kernel<V, OUT>), dim3(cdiv(total / V, 256)), dim3(256), 0, st, total, HW, K, comp,
                       area, cls, min_size, background, fill, best, out);
  else
    hipLaunchKernelGGL((cc_apply_kernel<1, OUT>), dim3(cdiv(total, 256)), dim3(256), 0, st, total, HW, K, comp, area,
                       cls, min_size, background, fill, best, out);
  return check_launch("cc_apply");
}

}  // namespace unet

using namespace unet;

extern "C" size_t unet_cc_workspace(long long N, int H, int W) {
  return cc_shape_ok(N, H, W) ? cc_best_bytes(N) + (size_t)N * H * W * sizeof(int) : 0;
}

extern "C" int unet_cc_label(long long N, int C, int K, int H, int W, const float* logits, const int64_t* labels,
                             const uint8_t* mask, int connectivity, int background, void* workspace, int32_t* comp,
                             int32_t* area, uint8_t* cls, int64_t* count, void* stream) {
  if (!cc_shape_ok(N, H, W)) {
    set_error("unet_cc_label: serves 1 <= H, W <= 4096 and N * H * W < 2^31");
    return UNET_ERR_UNSUPPORTED;
  }
  if (K < 1 || K > CC_MAXK || (logits != nullptr) + (labels != nullptr) + (mask != nullptr) != 1 ||
      (logits && C < 1) || (mask && K != 2) || (connectivity != 4 && connectivity != 8) || background < -1 ||
      background >= K || !workspace || !comp || !area || !cls || !count) {
    set_error("unet_cc_label: bad arguments (1 <= num_classes <= 16, one of logits / labels / mask, a mask has 2 "
              "classes, connectivity 4 or 8, -1 <= background < num_classes)");
    return UNET_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* parent = (int*)((char*)workspace + cc_best_bytes(N));
  unsigned long long* cnt = (unsigned long long*)count;
  const int tiles_x = cdiv(W, CC_T), tiles_y = cdiv(H, CC_T), conn8 = connectivity == 8;
  const long long total = N * H * W;
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(N * tiles_x * tiles_y)), dim3(256), 0, st, C, K, H, W, tiles_x,
                     tiles_y, logits, labels, mask, conn8, background, cls, parent, area, cnt);
  int rc = check_launch("cc_tile");
  if (rc) return rc;
  const int nvx = tiles_x - 1, nhy = tiles_y - 1;
  const long long seam = N * ((long long)nvx * H + (long long)nhy * W);
  if (seam > 0) {
    hipLaunchKernelGGL(cc_seam_kernel, dim3(cdiv(seam, 256)), dim3(256), 0, st, seam, H, W, nvx, nhy, conn8,
                       background, cls, parent);
    if ((rc = check_launch("cc_seam"))) return rc;
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, total, (unsigned)(H * W), K,
                     parent, cls, comp, area, cnt);
  return check_launch("cc_flatten");
}

extern "C" int unet_cc_filter(long long N, int K, int H, int W, const int32_t* comp, const int32_t* area,
                              const uint8_t* cls, long long min_size, int keep_largest, int background,
                              long long fill, void* workspace, int64_t* out_labels, uint8_t* out_mask,
                              void* stream) {
  if (!cc_shape_ok(N, H, W)) {
    set_error("unet_cc_filter: serves 1 <= H, W <= 4096 and N * H * W < 2^31");
    return UNET_ERR_UNSUPPORTED;
  }
  if (K < 1 || K > CC_MAXK || !comp || !area || !cls || background < -1 || background >= K || !workspace ||
      (out_labels != nullptr) + (out_mask != nullptr) != 1) {
    set_error("unet_cc_filter: bad arguments (1 <= num_classes <= 16, -1 <= background < num_classes, one of "
              "out_labels / out_mask)");
    return UNET_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long total = N * H * W;
  const unsigned HW = (unsigned)(H * W);
  unsigned long long* best = nullptr;
  if (keep_largest) {
    best = (unsigned long long*)workspace;
    hipLaunchKernelGGL(cc_clear_kernel, dim3(cdiv(N * K, 256)), dim3(256), 0, st, N * K, best);
    int rc = check_launch("cc_clear");
    if (rc) return rc;
    hipLaunchKernelGGL(cc_select_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, total, HW, K, comp, area, cls,
                       best);
    if ((rc = check_launch("cc_select"))) return rc;
  }
  return out_labels ? cc_launch_apply<int64_t>(st, total, HW, K, comp, area, cls, min_size, background, fill, best,
                                               out_labels)
                    : cc_launch_apply<uint8_t>(st, total, HW, K, comp, area, cls, min_size, background, fill, best,
                                               out_mask);
}
