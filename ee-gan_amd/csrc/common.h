// Shared device helpers for the EE-GAN MI355X (gfx950) kernel library.
// bf16 activations are stored as raw uint16 (NHWC, channel stride "ld");
// all arithmetic accumulates in fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

typedef uint16_t bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

#define EE_DEV __device__ __forceinline__
#define EE_HOST_DEV_INLINE __host__ __device__ __forceinline__

EE_DEV float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
EE_DEV bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN-preserving
  return __builtin_bit_cast(bf16_t, b);
}
EE_DEV uint32_t pack2(float a, float b) { return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16); }
EE_DEV float lo_f(uint32_t u) { return __uint_as_float(u << 16); }
EE_DEV float hi_f(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// activation codes shared with the host glue (eegan_hip/_lib.py)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_TANH = 3, ACT_SIGMOID = 4 };

EE_DEV float act_fwd(float v, int act, float slope) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_LRELU: return v > 0.f ? v : v * slope;
    case ACT_TANH: return tanhf(v);
    case ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    default: return v;
  }
}
// derivative expressed through the activation's OUTPUT y
EE_DEV float act_dgrad_from_y(float y, int act, float slope) {
  switch (act) {
    case ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case ACT_LRELU: return y > 0.f ? 1.f : slope;
    case ACT_TANH: return 1.f - y * y;
    case ACT_SIGMOID: return y * (1.f - y);
    default: return 1.f;
  }
}

EE_DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
EE_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block-wide sum for blockDim.x multiple of 64 (<= 1024); `red` >= 16 floats
EE_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  const int nw = blockDim.x >> 6;
  float t = (threadIdx.x < nw) ? red[threadIdx.x] : 0.f;
  if (w == 0) t = wave_sum(t);
  if (threadIdx.x == 0) red[0] = t;
  __syncthreads();
  float r = red[0];
  __syncthreads();
  return r;
}

static inline int ee_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int ee_round_up(int a, int b) { return (a + b - 1) / b * b; }

// "key=value,key=value" knob strings (EEGAN_CONV, EEGAN_BN): the integer after `key=` in `v`
// (the variable's value, may be null), `dflt` where the key is absent
static inline int ee_knob(const char* v, const char* key, int dflt) {
  if (!v) return dflt;
  const size_t n = strlen(key);
  for (const char* p = v; p && *p;) {
    if (!strncmp(p, key, n) && p[n] == '=') return atoi(p + n + 1);
    p = strchr(p, ',');
    if (p) ++p;
  }
  return dflt;
}

// error reporting (thread-local, no global mutable state shared across threads)
void ee_set_error(const char* fmt, ...);
int ee_check_launch(const char* what);

#define EE_LAUNCH_CHECK(name) return ee_check_launch(name)

// Launch-timing hook (the benchmark's roofline, eegan_timing_arm): while armed
// on this host thread, the next (up to two) kernels go through
// hipExtLaunchKernelGGL with start/stop events, which the runtime stamps at
// the dispatch's actual begin and end -- host launch gaps are not included.
struct EeTiming {
  hipEvent_t ev[4];
  int armed, used;
};
EeTiming& ee_timing();

template <typename F, typename... Args>
inline void ee_launch(F kernel, dim3 grid, dim3 block, uint32_t shm, hipStream_t s, Args... args) {
  EeTiming& t = ee_timing();
  if (t.armed && t.used < 2) {
    hipExtLaunchKernelGGL(kernel, grid, block, shm, s, t.ev[2 * t.used], t.ev[2 * t.used + 1], 0, args...);
    ++t.used;
  } else {
    kernel<<<grid, block, shm, s>>>(args...);
  }
}

// ---------------------------------------------------------------------------
// Deterministic column sums of row-major fp32 partials (split-K slabs, per-block
// statistics): out[y][map(c)] (+)= sum_{r < nrows} in[y*in_bstride + r*stride + c].
// Block = COLS columns x RG row groups; every group strides the rows, then
// the RG group sums are added in a fixed order, so results do not depend on
// scheduling.  RG follows nrows (1 / 8 / 32) so short sums waste no threads.
struct ColIdentity {
  EE_DEV long operator()(long c) const { return c; }
};

template <int COLS, int RG, typename Acc, typename Out, typename Map>
__global__ __launch_bounds__(COLS * RG) void colsum_rows_kernel(const float* __restrict__ in, int nrows, long ncols,
                                                               long stride, long in_bstride, Out* __restrict__ out,
                                                               long out_bstride, int accumulate, Map map) {
  __shared__ Acc sh[RG][COLS + 1];
  const int lane = threadIdx.x % COLS, g = threadIdx.x / COLS;
  const long c = blockIdx.x * (long)COLS + lane;
  in += blockIdx.y * in_bstride;
  out += blockIdx.y * out_bstride;
  Acc s = 0;
  if (c < ncols) {
    int r = g;
    // 8 rows' loads per round trip, summed in row order (as one at a time)
    for (; r + 7 * RG < nrows; r += 8 * RG) {
      float a[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = in[(long)(r + k * RG) * stride + c];
#pragma unroll
      for (int k = 0; k < 8; ++k) s += (Acc)a[k];
    }
    for (; r < nrows; r += RG) s += (Acc)in[(long)r * stride + c];
  }
  if (RG > 1) {
    sh[g][lane] = s;
    __syncthreads();
  }
  if (g == 0 && c < ncols) {
    Acc t = s;
    if (RG > 1) {
      t = 0;
#pragma unroll 8
      for (int i = 0; i < RG; ++i) t += sh[i][lane];
    }
    const long o = map(c);
    if (o >= 0) out[o] = accumulate ? (Out)(out[o] + (Out)t) : (Out)t;
  }
}

template <typename Acc, typename Out, typename Map = ColIdentity>
inline void launch_colsum(const float* in, int nrows, long ncols, long stride, long in_bstride, Out* out,
                          long out_bstride, int batches, int accumulate, hipStream_t s, Map map = Map()) {
  if (nrows <= 8) {
    dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)batches);
    ee_launch(colsum_rows_kernel<256, 1, Acc, Out, Map>, grid, dim3(256), 0, s, in, nrows, ncols, stride,
              in_bstride, out, out_bstride, accumulate, map);
  } else if (nrows <= 128) {
    dim3 grid((unsigned)((ncols + 31) / 32), (unsigned)batches);
    ee_launch(colsum_rows_kernel<32, 8, Acc, Out, Map>, grid, dim3(256), 0, s, in, nrows, ncols, stride,
              in_bstride, out, out_bstride, accumulate, map);
  } else {
    dim3 grid((unsigned)((ncols + 31) / 32), (unsigned)batches);
    ee_launch(colsum_rows_kernel<32, 32, Acc, Out, Map>, grid, dim3(1024), 0, s, in, nrows, ncols, stride,
              in_bstride, out, out_bstride, accumulate, map);
  }
}
