// What the text encoder's recurrence kernels (lstm_mfma.hip, gru_mfma.hip) share: a tile's caption
// lengths, the time a caption is at in a step, where a step's input-projection row comes from, and
// the entry points' shape check.  W is the row width: the gate columns, 4H for the LSTM, 3H for the GRU.
#pragma once
#include "common.h"

EE_DEV float sigmoid_f(float v) { return 1.f / (1.f + __expf(-v)); }

EE_DEV int clamp_len(long v, int T) { return (int)std::min<long>(std::max<long>(v, 1), T); }

// The clamped lengths of the M captions from n0 into Ls (0 for the rows past N: they never step);
// returns the maximum, which is uniform.
EE_DEV int tile_lengths(const long* __restrict__ lens, int n0, int N, int T, int M, int* Ls) {
  int Lmax = 0;
  for (int i = 0; i < M; ++i)
    if (n0 + i < N) Lmax = std::max(Lmax, clamp_len(lens[n0 + i], T));
  if ((int)threadIdx.x < M) Ls[threadIdx.x] = n0 + threadIdx.x < N ? clamp_len(lens[n0 + threadIdx.x], T) : 0;
  return Lmax;
}

// The time a caption of length L is at in step s of direction dir (0 once it has finished).
EE_DEV int step_time(int s, int L, int dir) { return s >= L ? 0 : dir == 0 ? s : L - 1 - s; }

// Where x_t W_ih^T + b of (row m of the workgroup's M captions, time t) comes from.  stage() runs
// once before the first barrier; row() is the W-float row.  Rows past N read some valid row.
//
// Eval mode: the projection depends on the token alone.  xtab [2][ntoken][W], ids [N][T]; the
// captions' tokens, clamped into the table, sit in LDS as toks [T][M].
template <int W>
struct TokenTable {
  const float* __restrict__ xtab;
  const long* __restrict__ ids;
  int ntoken;
  template <int M>
  EE_DEV void stage(int* toks, int n0, int N, int T) const {
    for (int i = threadIdx.x; i < M * T; i += 512) {
      const int m = i / T, t = i - m * T;
      const long tok = n0 + m < N ? ids[(long)(n0 + m) * T + t] : 0;
      toks[t * M + m] = (int)std::min<long>(std::max<long>(tok, 0), ntoken - 1);
    }
  }
  template <int M>
  EE_DEV const float* row(const int* toks, int dir, int n0, int N, int T, int m, int t) const {
    return xtab + ((long)dir * ntoken + toks[t * M + m]) * W;
  }
};

// Training: xproj [2][N*T][W], a row per (caption, t).
template <int W>
struct ProjRows {
  const float* __restrict__ xproj;
  template <int M>
  EE_DEV void stage(int*, int, int, int) const {}
  template <int M>
  EE_DEV const float* row(const int*, int dir, int n0, int N, int T, int m, int t) const {
    return xproj + (((long)dir * N + std::min(n0 + m, N - 1)) * T + t) * W;
  }
};

static inline int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

// H: the hidden size the kernels are built for
static inline int check_train_shape(const char* what, int N, int T, int Hdim, int Tout, int H) {
  if (Hdim != H) {
    ee_set_error("%s: H=%d, only %d is built", what, Hdim, H);
    return -22;
  }
  if (N < 1 || T < 1 || T > 128 || Tout < 1 || Tout > T) {
    ee_set_error("%s: N=%d T=%d Tout=%d", what, N, T, Tout);
    return -22;
  }
  return 0;
}
