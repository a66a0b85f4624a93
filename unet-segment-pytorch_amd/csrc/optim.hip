// optim.hip — the tail of the training step: gradient-norm clip + AdamW as three launches, ModelEMA as one.
//
// Reference: scripts/train.py:140-147 (clip_grad_norm_, optimizer.step, ema.update) and ModelEMA.update,
// unet/utils/general.py:156-184.  Stock torch runs these per tensor (AttentionUNet: 92 parameters, 90 buffers); here
// every tensor is one entry of a device segment table and every UNET_OPTIM_CHUNK elements of it one entry of a chunk
// map, and a launch has one workgroup per map entry.  The chunk of a workgroup comes from the map alone, so a sum
// never depends on the grid and the results are bit-identical from run to run (no atomics anywhere).
//
// All three streaming kernels are HBM-bound: per element the norm reads 4 bytes, the AdamW update reads 16 and
// writes 12, the EMA reads 8 and writes 4.  A lane owns one 16-byte vector per iteration (256 lanes x 16 B = one
// 4 KiB line-contiguous request per tensor per iteration), issues all loads of an iteration pair before any
// arithmetic, and an UNET_OPT_ALIGNED flag per segment (not a test per element) selects the 16-byte form; a segment
// with a misaligned pointer (a view at an odd storage offset) takes the element-wise form with the same coalescing.
#include <stdio.h>

#include "common.h"

namespace unet {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = UNET_OPTIM_CHUNK;
constexpr int OPT_VITERS = OPT_CHUNK / (OPT_THREADS * 4);   // 16-byte vectors per lane and chunk
constexpr int OPT_SITERS = OPT_CHUNK / OPT_THREADS;         // elements per lane and chunk, element-wise form
static_assert(OPT_CHUNK % (OPT_THREADS * 4) == 0 && OPT_VITERS % 2 == 0, "a chunk is whole iteration pairs");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// elements of this workgroup's chunk: [base, base + n) of its segment, n in [0, OPT_CHUNK]
__device__ __forceinline__ int chunk_extent(long long numel, int chunk, long long& base) {
  base = (long long)chunk * OPT_CHUNK;
  const long long left = numel - base;
  return left <= 0 ? 0 : (left < OPT_CHUNK ? (int)left : OPT_CHUNK);
}

// ------------------------------------------------------------------------------------------------
// pass 1: per-chunk sum of squares of the gradient
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void optim_gradnorm_kernel(const unet_optim_seg* __restrict__ segs,
                                                                     const unet_optim_chunk* __restrict__ map,
                                                                     double* __restrict__ partial) {
  __shared__ double wsum[OPT_THREADS / WAVE];
  const unet_optim_chunk cm = map[blockIdx.x];
  const unet_optim_seg s = segs[cm.seg];
  const int tid = threadIdx.x;
  float acc = 0.f;
  long long base;
  const int n = chunk_extent(s.numel, cm.chunk, base);
  if ((s.flags & UNET_OPT_KIND_MASK) == UNET_OPT_ADAMW && (s.flags & UNET_OPT_ACTIVE) && n > 0) {
    const float* g = (const float*)s.g + base;
    if (s.flags & UNET_OPT_ALIGNED) {
      const int n4 = n >> 2;
      float4 q[OPT_VITERS];
#pragma unroll
      for (int it = 0; it < OPT_VITERS; ++it) {
        const int i = it * OPT_THREADS + tid;
        q[it] = i < n4 ? reinterpret_cast<const float4*>(g)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < OPT_VITERS; ++it)
        acc += q[it].x * q[it].x + q[it].y * q[it].y + q[it].z * q[it].z + q[it].w * q[it].w;
      if (tid < (n & 3)) {
        const float t = g[4 * n4 + tid];
        acc += t * t;
      }
    } else {
#pragma unroll 8
      for (int it = 0; it < OPT_SITERS; ++it) {
        const int i = it * OPT_THREADS + tid;
        const float t = i < n ? g[i] : 0.f;
        acc += t * t;
      }
    }
  }
  const double w = wave_sum_f64((double)acc);
  if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = w;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < OPT_THREADS / WAVE; ++i) t += wsum[i];
    partial[blockIdx.x] = t;
  }
}

// ------------------------------------------------------------------------------------------------
// prepare: the scalars of the step (one workgroup)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void optim_prepare_kernel(
    const unet_optim_seg* __restrict__ segs, int nsegs, const unet_optim_group* __restrict__ groups,
    const double* __restrict__ partial, int nchunks, double max_norm, const float* __restrict__ grad_scale,
    const float* __restrict__ found_inf_in, double* __restrict__ bc, float* __restrict__ result) {
  __shared__ double red[OPT_THREADS];
  __shared__ int skip;
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int i = tid; i < nchunks; i += OPT_THREADS) a += partial[i];
  red[tid] = a;
  __syncthreads();
  for (int o = OPT_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    // GradScaler's own unscale multiplies by float(1 / double(scale))
    const double inv_scale = grad_scale ? (double)(float)(1.0 / (double)*grad_scale) : 1.0;
    const double total = nchunks > 0 ? sqrt(red[0]) * inv_scale : 0.0;
    const double clip = max_norm > 0.0 ? fmin(1.0, max_norm / (total + 1e-6)) : 1.0;
    const bool bad = (found_inf_in && *found_inf_in != 0.f) || !isfinite(total) || !isfinite(inv_scale);
    result[0] = (float)total;
    result[1] = bad ? 1.f : 0.f;
    result[2] = (float)(inv_scale * clip);
    skip = bad;
  }
  __syncthreads();
  if (skip) return;
  for (int i = tid; i < nsegs; i += OPT_THREADS) {
    const unet_optim_seg s = segs[i];
    if ((s.flags & UNET_OPT_KIND_MASK) != UNET_OPT_ADAMW || !(s.flags & UNET_OPT_ACTIVE)) continue;
    const float t = *s.step + 1.f;
    *s.step = t;
    const unet_optim_group gr = groups[s.group];
    bc[2 * i] = 1.0 / (1.0 - pow(gr.beta1, (double)t));
    bc[2 * i + 1] = 1.0 / sqrt(1.0 - pow(gr.beta2, (double)t));
  }
}

// ------------------------------------------------------------------------------------------------
// pass 2: the AdamW update
// ------------------------------------------------------------------------------------------------
struct AdamScalars {
  float coef, decay, w1, b2, w2, step_size, bc2s, eps;
};

__device__ __forceinline__ void adamw_elem(const AdamScalars& k, float& p, float g, float& m, float& v) {
  g *= k.coef;
  m = m + k.w1 * (g - m);
  v = k.b2 * v + k.w2 * (g * g);
  const float denom = __fsqrt_rn(v) * k.bc2s + k.eps;
  p = p * k.decay - k.step_size * __fdiv_rn(m, denom);
}

__global__ __launch_bounds__(OPT_THREADS) void optim_adamw_kernel(const unet_optim_seg* __restrict__ segs,
                                                                  const unet_optim_chunk* __restrict__ map,
                                                                  const unet_optim_group* __restrict__ groups,
                                                                  const double* __restrict__ bc,
                                                                  const float* __restrict__ result) {
  if (result[1] != 0.f) return;   // found_inf: parameters, moments and steps stay as they are
  const unet_optim_chunk cm = map[blockIdx.x];
  const unet_optim_seg s = segs[cm.seg];
  if ((s.flags & UNET_OPT_KIND_MASK) != UNET_OPT_ADAMW || !(s.flags & UNET_OPT_ACTIVE)) return;
  long long base;
  const int n = chunk_extent(s.numel, cm.chunk, base);
  if (n <= 0) return;
  const unet_optim_group gr = groups[s.group];
  const double lr = gr.lr_ptr ? (double)*gr.lr_ptr : gr.lr;
  AdamScalars k;   // each formed in double and rounded once, as torch forms its fp32 scalars from Python doubles
  k.coef = result[2];
  k.decay = (float)(1.0 - lr * gr.weight_decay);
  k.w1 = (float)(1.0 - gr.beta1);
  k.b2 = (float)gr.beta2;
  k.w2 = (float)(1.0 - gr.beta2);
  k.step_size = (float)(lr * bc[2 * cm.seg]);
  k.bc2s = (float)bc[2 * cm.seg + 1];
  k.eps = (float)gr.eps;
  const int tid = threadIdx.x;
  float* p = (float*)s.p + base;
  const float* g = (const float*)s.g + base;
  float* m = s.m + base;
  float* v = s.v + base;
  if (s.flags & UNET_OPT_ALIGNED) {
    const int n4 = n >> 2;
    // two 16-byte vectors of each of p, g, m, v in flight per lane before the arithmetic
    for (int it = 0; it < OPT_VITERS; it += 2) {
      const int i0 = it * OPT_THREADS + tid, i1 = i0 + OPT_THREADS;
      if (i0 >= n4) break;
      const bool two = i1 < n4;
      float4 P0 = reinterpret_cast<float4*>(p)[i0], G0 = reinterpret_cast<const float4*>(g)[i0];
      float4 M0 = reinterpret_cast<float4*>(m)[i0], V0 = reinterpret_cast<float4*>(v)[i0];
      float4 P1 = P0, G1 = G0, M1 = M0, V1 = V0;
      if (two) {
        P1 = reinterpret_cast<float4*>(p)[i1];
        G1 = reinterpret_cast<const float4*>(g)[i1];
        M1 = reinterpret_cast<float4*>(m)[i1];
        V1 = reinterpret_cast<float4*>(v)[i1];
      }
      adamw_elem(k, P0.x, G0.x, M0.x, V0.x);
      adamw_elem(k, P0.y, G0.y, M0.y, V0.y);
      adamw_elem(k, P0.z, G0.z, M0.z, V0.z);
      adamw_elem(k, P0.w, G0.w, M0.w, V0.w);
      reinterpret_cast<float4*>(p)[i0] = P0;
      reinterpret_cast<float4*>(m)[i0] = M0;
      reinterpret_cast<float4*>(v)[i0] = V0;
      if (two) {
        adamw_elem(k, P1.x, G1.x, M1.x, V1.x);
        adamw_elem(k, P1.y, G1.y, M1.y, V1.y);
        adamw_elem(k, P1.z, G1.z, M1.z, V1.z);
        adamw_elem(k, P1.w, G1.w, M1.w, V1.w);
        reinterpret_cast<float4*>(p)[i1] = P1;
        reinterpret_cast<float4*>(m)[i1] = M1;
        reinterpret_cast<float4*>(v)[i1] = V1;
      }
    }
    if (tid < (n & 3)) {
      const int i = 4 * n4 + tid;
      float P = p[i], M = m[i], V = v[i];
      adamw_elem(k, P, g[i], M, V);
      p[i] = P; m[i] = M; v[i] = V;
    }
  } else {
    for (int it = 0; it < OPT_SITERS; ++it) {
      const int i = it * OPT_THREADS + tid;
      if (i >= n) break;
      float P = p[i], M = m[i], V = v[i];
      adamw_elem(k, P, g[i], M, V);
      p[i] = P; m[i] = M; v[i] = V;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// ModelEMA.update: averaged parameters and copied buffers in one launch
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void ema_update_kernel(const unet_optim_seg* __restrict__ segs,
                                                                 const unet_optim_chunk* __restrict__ map, float d,
                                                                 float omd) {
  const unet_optim_chunk cm = map[blockIdx.x];
  const unet_optim_seg s = segs[cm.seg];
  const int kind = s.flags & UNET_OPT_KIND_MASK;
  const int tid = threadIdx.x;
  if (kind == UNET_OPT_EMA) {
    long long base;
    const int n = chunk_extent(s.numel, cm.chunk, base);
    if (n <= 0) return;
    float* e = (float*)s.p + base;
    const float* p = (const float*)s.g + base;
    if (s.flags & UNET_OPT_ALIGNED) {
      const int n4 = n >> 2;
      float4 E[OPT_VITERS], P[OPT_VITERS];
#pragma unroll
      for (int it = 0; it < OPT_VITERS; ++it) {
        const int i = it * OPT_THREADS + tid;
        if (i < n4) {
          E[it] = reinterpret_cast<float4*>(e)[i];
          P[it] = reinterpret_cast<const float4*>(p)[i];
        }
      }
#pragma unroll
      for (int it = 0; it < OPT_VITERS; ++it) {
        const int i = it * OPT_THREADS + tid;
        if (i < n4)
          reinterpret_cast<float4*>(e)[i] = make_float4(d * E[it].x + omd * P[it].x, d * E[it].y + omd * P[it].y,
                                                        d * E[it].z + omd * P[it].z, d * E[it].w + omd * P[it].w);
      }
      if (tid < (n & 3)) {
        const int i = 4 * n4 + tid;
        e[i] = d * e[i] + omd * p[i];
      }
    } else {
      for (int it = 0; it < OPT_SITERS; ++it) {
        const int i = it * OPT_THREADS + tid;
        if (i >= n) break;
        e[i] = d * e[i] + omd * p[i];
      }
    }
  } else if (kind == UNET_OPT_COPY) {
    // numel is bytes; a chunk is 4 * OPT_CHUNK of them, so a chunk of an aligned segment starts 16-byte aligned
    const long long base = (long long)cm.chunk * (4LL * OPT_CHUNK);
    const long long left = s.numel - base;
    if (left <= 0) return;
    const int n = left < 4LL * OPT_CHUNK ? (int)left : 4 * OPT_CHUNK;
    unsigned char* dst = (unsigned char*)s.p + base;
    const unsigned char* src = (const unsigned char*)s.g + base;
    int done = 0;
    if (s.flags & UNET_OPT_ALIGNED) {
      const int n16 = n >> 4;
#pragma unroll
      for (int it = 0; it < OPT_VITERS; ++it) {
        const int i = it * OPT_THREADS + tid;
        if (i < n16) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
      }
      done = n16 << 4;
    }
    for (int i = done + tid; i < n; i += OPT_THREADS) dst[i] = src[i];   // the tail, or a misaligned segment
  }
}

}  // namespace unet

using namespace unet;

extern "C" int unet_optim_chunks(long long numel) {
  const long long c = (numel + OPT_CHUNK - 1) / OPT_CHUNK;
  return c < 1 ? 1 : (int)c;
}

static int optim_table_ok(const char* who, const void* segs, const void* map, int nchunks) {
  if (!segs || !map || nchunks <= 0) {
    static thread_local char msg[96];
    snprintf(msg, sizeof(msg), "%s: needs a segment table and a chunk map of at least one entry", who);
    set_error(msg);
    return 0;
  }
  return 1;
}

extern "C" int unet_optim_gradnorm(const unet_optim_seg* segs, const unet_optim_chunk* map, int nchunks,
                                   double* partial, void* stream) {
  if (!optim_table_ok("unet_optim_gradnorm", segs, map, nchunks) || !partial) {
    if (segs && map && nchunks > 0) set_error("unet_optim_gradnorm: partial is NULL");
    return UNET_ERR_ARG;
  }
  hipLaunchKernelGGL(optim_gradnorm_kernel, dim3(nchunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, segs, map,
                     partial);
  return check_launch("optim_gradnorm");
}

extern "C" int unet_optim_prepare(const unet_optim_seg* segs, int nsegs, const unet_optim_group* groups,
                                  const double* partial, int nchunks, double max_norm, const float* grad_scale,
                                  const float* found_inf_in, double* bc, float* result, void* stream) {
  if (!segs || nsegs <= 0 || !groups || nchunks < 0 || (nchunks > 0 && !partial) || !bc || !result) {
    set_error("unet_optim_prepare: bad arguments (table, groups, bc and result are required; partial when nchunks > 0)");
    return UNET_ERR_ARG;
  }
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, segs, nsegs, groups,
                     partial, nchunks, max_norm, grad_scale, found_inf_in, bc, result);
  return check_launch("optim_prepare");
}

extern "C" int unet_optim_adamw(const unet_optim_seg* segs, const unet_optim_chunk* map, int nchunks,
                                const unet_optim_group* groups, const double* bc, const float* result,
                                void* stream) {
  if (!optim_table_ok("unet_optim_adamw", segs, map, nchunks) || !groups || !bc || !result) {
    if (segs && map && nchunks > 0) set_error("unet_optim_adamw: groups, bc and result are required");
    return UNET_ERR_ARG;
  }
  hipLaunchKernelGGL(optim_adamw_kernel, dim3(nchunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, segs, map, groups,
                     bc, result);
  return check_launch("optim_adamw");
}

extern "C" int unet_ema_update(const unet_optim_seg* segs, const unet_optim_chunk* map, int nchunks, float decay,
                               float one_minus_decay, void* stream) {
  if (!optim_table_ok("unet_ema_update", segs, map, nchunks)) return UNET_ERR_ARG;
  hipLaunchKernelGGL(ema_update_kernel, dim3(nchunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, segs, map, decay,
                     one_minus_decay);
  return check_launch("ema_update");
}
