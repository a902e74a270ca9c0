// Frechet distance on the device (reference metrics/FID/fid_score.py:189-228):
//   d^2 = |mu1 - mu2|^2 + Tr(C1) + Tr(C2) - 2 Tr(sqrt(C1 C2)).
// Only the trace of the root is needed, so instead of the reference's Schur
// square root (scipy.linalg.sqrtm, host) the coupled Newton-Schulz iteration
// runs on A = C1 C2 with fp64 matrix instructions:
//   s = |A|_F, Y0 = A / s, Z0 = I;  T = 1.5 I - 0.5 Z Y;  Y' = Y T;  Z' = T Z;
//   Tr(sqrt(A)) ~ sqrt(s) Tr(Y).
//
//  * fid_dgemm_kernel: C = alpha A B + beta I on square row-major matrices
//    whose side P is a multiple of 128.  One 128 x 128 output tile per
//    workgroup (P = 2048: 256 tiles, one per CU), 256 threads = 2 x 2 waves of
//    64 x 64, i.e. 4 x 4 v_mfma_f64_16x16x4_f64 blocks of 4 doubles per lane
//    (128 accumulator registers).  K goes through LDS in 16-deep slabs, both
//    operands k-major ([k][128]), double buffered: 2 x 2 x 16 KB, the whole
//    64 KB a workgroup may declare.  The next slab is fetched into registers
//    before the current one is multiplied and stored after it, so one barrier
//    per slab suffices.  The MFMA operand reads (A: row = lane % 16, k =
//    lane / 16; B: k = lane / 16, col = lane % 16) are 4 runs of 16 doubles;
//    odd k rows have their 16-column groups swapped in pairs (column ^ 16),
//    which puts neighbouring k on opposite halves of the 64 banks without the
//    padding that would not fit.  blockIdx.z picks one of two independent
//    products (Y' and Z' of one iteration share a launch).
//    Epilogues: beta on the diagonal; per-tile sum of c^2 or of the diagonal,
//    written to the tile's own slot and added up in slot order by
//    fid_finish_kernel -- no atomics, two runs are bit-identical.
//  * small kernels: zero-padded copy (+ eps on the diagonal, also the identity
//    Z0), the 1 / s scaling from the device scalar, the final combination.
//  * eegan_fid_frechet drives the iteration and reads Tr(Y) back once per
//    iteration for the stopping rule, so it synchronises the stream every
//    iteration: an evaluation path, not capturable in a graph.
//    It stops when |dTr| <= 1e-11 |Tr|.  Short of that it remembers the trace
//    with the smallest |dTr| among those below 1e-6 |Tr| and goes on: late
//    small eigenvalues make |dTr| rise for a few steps and fall again (a
//    full-rank D = 272 product dips to 4.5e-8, rises to 6.9e-8 and converges 7
//    iterations later; stopping at the dip leaves 2e-7), while at the
//    round-off floor of an ill-conditioned product the rise never ends: Z
//    grows ~1.5x per step on the null space of a rank-deficient A and a fixed
//    long iteration count ends in NaN.  So when |dTr| climbs back above
//    1e-6 |Tr|, the trace stops being finite, or the cap of 64 iterations is
//    reached, the remembered trace is the result.  With nothing remembered
//    the pass has failed: a non-finite one is retried once with eps on both
//    diagonals (the reference's fallback), anything else is an error.  There
//    is no host fallback.
#include <math.h>

#include "common.h"
#include "../../include/eegan_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;
typedef __attribute__((ext_vector_type(2))) double f64x2_t;

constexpr int FT = 128;        // output tile
constexpr int FK = 16;         // K slab
constexpr int FID_MAX_D = 8192;
constexpr int FID_MAX_IT = 64;
constexpr int SC_S = 0, SC_INV = 1, SC_TR = 8;   // scalar slots: |A|_F, 1 / |A|_F, Tr(Y) of iteration i at SC_TR + i
constexpr int SC_N = 128;

enum { EPI_PLAIN = 0, EPI_SUMSQ = 1, EPI_TRACE = 2 };

struct DgemmJob {
  const double* A;
  const double* B;
  double* C;
  double* part;   // per-tile partials (EPI_SUMSQ / EPI_TRACE), tiles x tiles
  double alpha, beta;
  int epi;
};
struct DgemmJobs {
  DgemmJob j[2];
};

// LDS offset of (k, c) in a [FK][FT] slab
EE_DEV int slab_at(int k, int c) { return k * FT + (c ^ ((k & 1) << 4)); }

EE_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void fid_dgemm_kernel(DgemmJobs jobs, int P) {
  __shared__ double sA[2][FK * FT], sB[2][FK * FT];
  const DgemmJob jb = jobs.j[blockIdx.z];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const int i0 = blockIdx.y * FT, j0 = blockIdx.x * FT;
  // global -> LDS: A row ar, k ak .. ak + 7 (transposed on the way in);
  // B row bk, columns bc .. bc + 7
  const int ar = tid & 127, ak = (tid >> 7) * 8;
  const int bk = tid >> 4, bc = (tid & 15) * 8;
  const double* ga = jb.A + (long)(i0 + ar) * P + ak;
  const double* gb = jb.B + (long)bk * P + j0 + bc;
  f64x2_t ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ra[q] = *(const f64x2_t*)(ga + k0 + 2 * q);
      rb[q] = *(const f64x2_t*)(gb + (long)k0 * P + 2 * q);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sA[buf][slab_at(ak + 2 * q, ar)] = ra[q].x;
      sA[buf][slab_at(ak + 2 * q + 1, ar)] = ra[q].y;
      *(f64x2_t*)&sB[buf][slab_at(bk, bc + 2 * q)] = rb[q];
    }
  };
  f64x4_t acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  const int nslab = P / FK;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < nslab;
    if (more) fetch((s + 1) * FK);
#pragma unroll
    for (int kk = 0; kk < FK; kk += 4) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = sA[buf][slab_at(kk + lk, wm * 64 + u * 16 + lr)];
        b[u] = sB[buf][slab_at(kk + lk, wn * 64 + u * 16 + lr)];
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
    }
    // buf ^ 1 was last read before the previous barrier
    if (more) stage(buf ^ 1);
    __syncthreads();
  }
  // accumulator element r of lane: row 4 * r + lane / 16, column lane % 16 of the 16 x 16 block
  // (the fp64 blocks interleave rows over the registers, unlike the fp32 16x16x4 map)
  double red = 0.0;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + wm * 64 + m * 16 + 4 * r + lk, gj = j0 + wn * 64 + n * 16 + lr;
        const double v = jb.alpha * acc[m][n][r] + (gi == gj ? jb.beta : 0.0);
        jb.C[(long)gi * P + gj] = v;
        if (jb.epi == EPI_SUMSQ) red = fma(v, v, red);
        if (jb.epi == EPI_TRACE && gi == gj) red += v;
      }
  if (jb.epi != EPI_PLAIN) {   // uniform per workgroup; the slabs are free after the loop's last barrier
    red = wave_sum_f64(red);
    if (lane == 0) sA[0][wave] = red;
    __syncthreads();
    if (tid == 0) jb.part[blockIdx.y * gridDim.x + blockIdx.x] = ((sA[0][0] + sA[0][1]) + sA[0][2]) + sA[0][3];
  }
}

// block-wide fp64 sum in a fixed order (256 threads); the result is valid in thread 0
EE_DEV double block_sum_f64(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < 256; ++i) t += sh[i];
  return t;
}

// sum of the n per-tile partials in slot order; mode EPI_SUMSQ: scal[SC_S] = sqrt, scal[SC_INV] = 1 / sqrt;
// EPI_TRACE: scal[slot] = sum
__global__ __launch_bounds__(256) void fid_finish_kernel(const double* __restrict__ part, int n, int mode, int slot,
                                                         double* __restrict__ scal) {
  __shared__ double sh[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) v += part[i];
  const double t = block_sum_f64(v, sh);
  if (threadIdx.x == 0) {
    if (mode == EPI_SUMSQ) {
      const double s = sqrt(t);
      scal[SC_S] = s;
      scal[SC_INV] = 1.0 / s;
    } else {
      scal[slot] = t;
    }
  }
}

// dst [P][P] = src [D][D] (zeros when src is null) + eps on the first D diagonal elements, zero outside D x D
__global__ __launch_bounds__(256) void fid_pad_kernel(const double* __restrict__ src, int D, int P, double eps,
                                                      double* __restrict__ dst) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)P * P) return;
  const int i = (int)(e / P), j = (int)(e % P);
  double v = 0.0;
  if (i < D && j < D) v = (src ? src[(long)i * D + j] : 0.0) + (i == j ? eps : 0.0);
  dst[e] = v;
}

__global__ __launch_bounds__(256) void fid_unpad_kernel(const double* __restrict__ src, int D, int P,
                                                        double* __restrict__ dst) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)D * D) return;
  dst[e] = src[(e / D) * P + e % D];
}

__global__ __launch_bounds__(256) void fid_scale_kernel(double* __restrict__ y, long n,
                                                        const double* __restrict__ scal) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) y[e] *= scal[SC_INV];
}

// out = {d^2, Tr(sqrt(C1 C2)), iterations, eps retry taken}
__global__ __launch_bounds__(256) void fid_frechet_final_kernel(const double* __restrict__ mu1,
                                                                const double* __restrict__ c1,
                                                                const double* __restrict__ mu2,
                                                                const double* __restrict__ c2, int D,
                                                                const double* __restrict__ scal, int slot, int iters,
                                                                int retried, double* __restrict__ out) {
  __shared__ double sh[256];
  double dm = 0.0, t1 = 0.0, t2 = 0.0;
  for (int i = threadIdx.x; i < D; i += 256) {
    const double d = mu1[i] - mu2[i];
    dm = fma(d, d, dm);
    t1 += c1[(long)i * D + i];
    t2 += c2[(long)i * D + i];
  }
  dm = block_sum_f64(dm, sh);
  t1 = block_sum_f64(t1, sh);
  t2 = block_sum_f64(t2, sh);
  if (threadIdx.x == 0) {
    const double root = sqrt(scal[SC_S]) * scal[slot];
    out[0] = dm + t1 + t2 - 2.0 * root;
    out[1] = root;
    out[2] = (double)iters;
    out[3] = (double)retried;
  }
}

inline int pad_of(int D) { return (D + FT - 1) / FT * FT; }

int launch_dgemm(const DgemmJobs& jobs, int njobs, int P, hipStream_t s) {
  ee_launch(fid_dgemm_kernel, dim3(P / FT, P / FT, njobs), dim3(256), 0, s, jobs, P);
  return ee_check_launch("fid_dgemm");
}

int launch_pad(const double* src, int D, int P, double eps, double* dst, hipStream_t s) {
  ee_launch(fid_pad_kernel, dim3((unsigned)(((long)P * P + 255) / 256)), dim3(256), 0, s, src, D, P, eps, dst);
  return ee_check_launch("fid_pad");
}

int read_f64(const double* dev, int n, double* host, hipStream_t s, const char* what) {
  hipError_t e = hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    ee_set_error("%s: %s", what, hipGetErrorString(e));
    return -(int)e;
  }
  return 0;
}

// One pass of the iteration with `eps` on both diagonals.  Returns 0 with out[] written, 1 when the result is
// not finite, 2 when the cap was hit, < 0 on a runtime error.
int frechet_pass(const double* mu1, const double* c1, const double* mu2, const double* c2, int D, double eps,
                 int retried, double* out, double* ws, hipStream_t s) {
  const int P = pad_of(D), nt = P / FT;
  const long pp = (long)P * P;
  double* buf[5] = {ws, ws + pp, ws + 2 * pp, ws + 3 * pp, ws + 4 * pp};
  double* part = ws + 5 * pp;
  double* scal = part + (long)nt * nt;
  int rc;
  if ((rc = launch_pad(c1, D, P, eps, buf[0], s))) return rc;
  if ((rc = launch_pad(c2, D, P, eps, buf[1], s))) return rc;
  DgemmJobs jobs = {};
  jobs.j[0] = {buf[0], buf[1], buf[2], part, 1.0, 0.0, EPI_SUMSQ};   // A = C1 C2, |A|_F^2 per tile
  if ((rc = launch_dgemm(jobs, 1, P, s))) return rc;
  ee_launch(fid_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nt * nt, (int)EPI_SUMSQ, 0, scal);
  if ((rc = ee_check_launch("fid_finish"))) return rc;
  double *Y = buf[2], *Z = buf[3], *T = buf[4], *Yn = buf[0], *Zn = buf[1];
  ee_launch(fid_scale_kernel, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, s, Y, pp, (const double*)scal);
  if ((rc = ee_check_launch("fid_scale"))) return rc;
  if ((rc = launch_pad(nullptr, D, P, 1.0, Z, s))) return rc;
  double prev = 0.0, best_d = HUGE_VAL;
  int use = 0, best = 0, iters = 0;
  bool finite = true;
  for (int it = 1; it <= FID_MAX_IT && !use; ++it) {
    jobs.j[0] = {Z, Y, T, nullptr, -0.5, 1.5, EPI_PLAIN};
    if ((rc = launch_dgemm(jobs, 1, P, s))) return rc;
    jobs.j[0] = {Y, T, Yn, part, 1.0, 0.0, EPI_TRACE};
    jobs.j[1] = {T, Z, Zn, nullptr, 1.0, 0.0, EPI_PLAIN};
    if ((rc = launch_dgemm(jobs, 2, P, s))) return rc;
    ee_launch(fid_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nt * nt, (int)EPI_TRACE, SC_TR + it,
              scal);
    if ((rc = ee_check_launch("fid_finish"))) return rc;
    std::swap(Y, Yn);
    std::swap(Z, Zn);
    double tr;
    if ((rc = read_f64(scal + SC_TR + it, 1, &tr, s, "fid_frechet: trace readback"))) return rc;
    iters = it;
    if (!isfinite(tr)) {
      finite = false;
      break;
    }
    if (it > 1) {
      const double d = fabs(tr - prev);
      if (d <= 1e-11 * fabs(tr)) {
        use = it;
      } else if (d <= 1e-6 * fabs(tr)) {
        if (d < best_d) best_d = d, best = it;
      } else if (best) {
        break;   // past the round-off floor
      }
    }
    prev = tr;
  }
  if (!use) use = best;
  if (!use) return finite ? 2 : 1;
  ee_launch(fid_frechet_final_kernel, dim3(1), dim3(256), 0, s, mu1, c1, mu2, c2, D, (const double*)scal, SC_TR + use,
            iters, retried, out);
  if ((rc = ee_check_launch("fid_frechet_final"))) return rc;
  double d2;
  if ((rc = read_f64(out, 1, &d2, s, "fid_frechet: result readback"))) return rc;
  return isfinite(d2) ? 0 : 1;
}

}  // namespace

extern "C" {

long eegan_fid_frechet_workspace(int D) {
  if (D < 1 || D > FID_MAX_D) return 0;
  const long P = pad_of(D), nt = P / FT;
  return (5 * P * P + nt * nt + SC_N) * (long)sizeof(double);
}

int eegan_fid_frechet(const double* mu1, const double* sigma1, const double* mu2, const double* sigma2, int D,
                      double eps, double* out, void* ws, hipStream_t s) {
  if (D < 1 || D > FID_MAX_D) {
    ee_set_error("fid_frechet: need 1 <= D <= %d (D=%d)", FID_MAX_D, D);
    return -22;
  }
  int rc = frechet_pass(mu1, sigma1, mu2, sigma2, D, 0.0, 0, out, (double*)ws, s);
  if (rc == 1) rc = frechet_pass(mu1, sigma1, mu2, sigma2, D, eps, 1, out, (double*)ws, s);
  if (rc == 1) ee_set_error("fid_frechet: Tr(sqrt(C1 C2)) is not finite, with eps=%g on the diagonals as well", eps);
  if (rc == 2) ee_set_error("fid_frechet: Newton-Schulz did not converge in %d iterations (D=%d)", FID_MAX_IT, D);
  return rc > 0 ? -34 : rc;
}

int eegan_fid_dgemm(const double* A, const double* B, int D, double alpha, double beta_diag, double* C,
                    hipStream_t s) {
  if (D < 1 || D > FID_MAX_D) {
    ee_set_error("fid_dgemm: need 1 <= D <= %d (D=%d)", FID_MAX_D, D);
    return -22;
  }
  const int P = pad_of(D);
  const long pp = (long)P * P;
  double* tmp = nullptr;
  hipError_t e = hipMalloc((void**)&tmp, 3 * pp * sizeof(double));
  if (e != hipSuccess) {
    ee_set_error("fid_dgemm: padded operands: %s", hipGetErrorString(e));
    return -(int)e;
  }
  int rc = launch_pad(A, D, P, 0.0, tmp, s);
  if (!rc) rc = launch_pad(B, D, P, 0.0, tmp + pp, s);
  if (!rc) {
    DgemmJobs jobs = {};
    jobs.j[0] = {tmp, tmp + pp, tmp + 2 * pp, nullptr, alpha, beta_diag, EPI_PLAIN};
    rc = launch_dgemm(jobs, 1, P, s);
  }
  if (!rc) {
    ee_launch(fid_unpad_kernel, dim3((unsigned)(((long)D * D + 255) / 256)), dim3(256), 0, s,
              (const double*)(tmp + 2 * pp), D, P, C);
    rc = ee_check_launch("fid_unpad");
  }
  e = hipStreamSynchronize(s);   // the temporaries are freed below
  (void)hipFree(tmp);
  if (!rc && e != hipSuccess) {
    ee_set_error("fid_dgemm: %s", hipGetErrorString(e));
    rc = -(int)e;
  }
  return rc;
}

}  // extern "C"
