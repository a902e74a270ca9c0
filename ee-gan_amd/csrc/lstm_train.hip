// Trainable DAMSM text encoder (RNN_ENCODER, DAMSM.py:88-115): the bi-LSTM
// recurrence forward with a tape, its back-propagation through time, and the
// embedding gather / gradient with the dropout keep-mask fused in.  fp32
// throughout, no atomics: every output element has one writer and every sum a
// fixed order, so two calls on the same inputs give the same bits.
//
// Both recurrence kernels use lstm_sent_kernel<1>'s split (lstm_batched.hip):
// a workgroup of 8 waves owns 16 captions of one direction and wave w owns
// hidden units 16w..16w+15.  (caption 4q + r of the tile, unit u = 16w + lane%16)
// sits in lane (q, lane%16), register r of every accumulator tile, forward and
// backward, so the cell arithmetic and the tape traffic are register-only.
//
// forward:  gates[16 x 4H] = h[16 x H] . W_hh^T; the wave's 128 x 64 slice of
//           W_hh^T is the resident B operand (128 VGPRs), h goes through the
//           padded double-buffered LDS array, one barrier per step.
// backward: dh[16 x H] = dgates[16 x 4H] . W_hh; the wave's 512 x 16 slice of
//           W_hh is the resident B operand (128 VGPRs), dgates goes through one
//           padded LDS array, two barriers per step.
//
// tape [2][tiles][T steps][5: i f g o c][8 waves][4 r][64 lanes]: the
// accumulator order, so a wave stores and reloads each value as 256 B runs.
#include "common.h"
#include "../../include/eegan_hip.h"

namespace {

constexpr int H = 128;        // hidden units per direction (the DAMSM configs' only value)
constexpr int G = 4 * H;      // gate columns
constexpr int LDH = H + 4;    // h rows: 16 rows' float4 reads start 4 banks apart
constexpr int LDG = G + 4;    // dgates rows: 516 % 64 = 4, the same spread
constexpr int KS = H / 4;     // forward MFMA k-steps
constexpr int KB = G / 4;     // backward MFMA k-steps
constexpr int TV = 8 * 4 * 64;  // floats of one tape value of one (direction, tile, step)

EE_DEV float sigmoid_f(float v) { return 1.f / (1.f + __expf(-v)); }

EE_DEV int clamp_len(long v, int T) { return (int)std::min<long>(std::max<long>(v, 1), T); }

// The tile's clamped lengths into Ls (0 for the rows past N: they never step); returns the maximum.
EE_DEV int tile_lengths(const long* __restrict__ lens, int n0, int N, int T, int* Ls) {
  int Lmax = 0;
  for (int i = 0; i < 16; ++i)
    if (n0 + i < N) Lmax = std::max(Lmax, clamp_len(lens[n0 + i], T));
  if (threadIdx.x < 16) Ls[threadIdx.x] = n0 + threadIdx.x < N ? clamp_len(lens[n0 + threadIdx.x], T) : 0;
  return Lmax;
}

// xproj [2][N*T][4H] (bias included), whh [2][8 waves][KS][4 gates][64 lanes] (as lstm_sent_kernel's),
// lens [N]; words [N][2H][Tout], sent [N][2H], tape (above), hprev [2][N*T][H]
__global__ __launch_bounds__(512) void lstm_train_fwd_kernel(const float* __restrict__ xproj,
                                                             const float* __restrict__ whh,
                                                             const long* __restrict__ lens, int N, int T, int Tout,
                                                             float* __restrict__ words, float* __restrict__ sent,
                                                             float* __restrict__ tape, float* __restrict__ hprev) {
  __shared__ __attribute__((aligned(16))) float hs[2][16][LDH];
  __shared__ int Ls[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, col = lane & 15;
  const int dir = blockIdx.y;
  const int n0 = blockIdx.x * 16;
  const int u = 16 * w + col;  // this lane's hidden unit

  // the wave's W_hh^T slice, once
  float bw[KS][4];
  {
    const float* wp = whh + ((long)(dir * 8 + w) * KS * 4) * 64 + lane;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int g = 0; g < 4; ++g) bw[s][g] = wp[(s * 4 + g) * 64];
  }

  const int Lmax = tile_lengths(lens, n0, N, T, Ls);
  for (int i = threadIdx.x; i < 2 * 16 * LDH; i += 512) (&hs[0][0][0])[i] = 0.f;
  __syncthreads();

  // what no step writes: words and the h_prev rows past each caption's length
  for (int i = threadIdx.x; i < 16 * H * Tout; i += 512) {
    const int m = i / (H * Tout), k = i / Tout % H, t = i % Tout;
    if (n0 + m < N && t >= Ls[m]) words[((long)(n0 + m) * 2 * H + dir * H + k) * Tout + t] = 0.f;
  }
  for (int i = threadIdx.x; i < 16 * T * H; i += 512) {
    const int m = i / (T * H), t = i / H % T, k = i % H;
    if (n0 + m < N && t >= Ls[m]) hprev[(((long)dir * N + n0 + m) * T + t) * H + k] = 0.f;
  }

  // per register r: the caption's length, its (clamped) row and its tape slot
  int Lr[4];
  long nr[4], rowr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Lr[r] = Ls[4 * q + r];
    nr[r] = std::min(n0 + 4 * q + r, N - 1);
    rowr[r] = ((long)dir * N + nr[r]) * T;
  }
  float* tp = tape + (((long)dir * gridDim.x + blockIdx.x) * T * 5 * 8 + w) * 256 + lane;

  float c[4], hv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = hv[r] = 0.f;

  int cur = 0;
  for (int s = 0; s < Lmax; ++s) {
    // this step's projection rows are requested first and added after the MFMA chain, which hides them
    f32x4_t x[4], acc[4];
    int tr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool run = s < Lr[r];
      tr[r] = !run ? 0 : dir == 0 ? s : Lr[r] - 1 - s;
      const float* row = xproj + (rowr[r] + tr[r]) * G + u;
#pragma unroll
      for (int g = 0; g < 4; ++g) x[g][r] = row[g * H];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f32x4_t a = *(const f32x4_t*)&hs[cur][col][16 * s4 + 4 * q];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bw[s4 * 4 + j][g], acc[g], 0, 0, 0);
    }

    float* ts = tp + (long)s * 5 * TV;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool run = s < Lr[r];  // a select: the MFMAs need the whole wave
      const float ig = sigmoid_f(x[0][r] + acc[0][r]);
      const float fg = sigmoid_f(x[1][r] + acc[1][r]);
      const float gg = tanhf(x[2][r] + acc[2][r]);
      const float og = sigmoid_f(x[3][r] + acc[3][r]);
      const float cn = __fmaf_rn(fg, c[r], ig * gg);
      const float hn = og * tanhf(cn);
      if (run) hprev[(rowr[r] + tr[r]) * H + u] = hv[r];
      c[r] = run ? cn : c[r];
      hv[r] = run ? hn : hv[r];
      ts[0 * TV + r * 64] = ig;
      ts[1 * TV + r * 64] = fg;
      ts[2 * TV + r * 64] = gg;
      ts[3 * TV + r * 64] = og;
      ts[4 * TV + r * 64] = c[r];
      hs[cur ^ 1][4 * q + r][u] = hv[r];
      if (run && tr[r] < Tout) words[(nr[r] * 2 * H + dir * H + u) * Tout + tr[r]] = hn;
    }
    __syncthreads();
    cur ^= 1;
  }

  // the last buffer holds every row's h at its own last step
  for (int i = threadIdx.x; i < 16 * H; i += 512) {
    const int m = i / H, k = i % H;
    if (n0 + m < N) sent[(long)(n0 + m) * 2 * H + dir * H + k] = hs[cur][m][k];
  }
}

// dwords [N][2H][Tout], dsent [N][2H], wbk [2][8 waves][KB][64 lanes] (W_hh, not transposed), lens [N],
// tape as written by the forward; dxproj [2][N*T][4H]
__global__ __launch_bounds__(512) void lstm_train_bwd_kernel(const float* __restrict__ dwords,
                                                             const float* __restrict__ dsent,
                                                             const float* __restrict__ wbk,
                                                             const long* __restrict__ lens,
                                                             const float* __restrict__ tape, int N, int T, int Tout,
                                                             float* __restrict__ dxproj) {
  __shared__ __attribute__((aligned(16))) float dg[16][LDG];
  __shared__ int Ls[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, col = lane & 15;
  const int dir = blockIdx.y;
  const int n0 = blockIdx.x * 16;
  const int u = 16 * w + col;

  // the wave's 512 x 16 slice of W_hh, once
  float bw[KB];
  {
    const float* wp = wbk + ((long)(dir * 8 + w) * KB) * 64 + lane;
#pragma unroll
    for (int s = 0; s < KB; ++s) bw[s] = wp[s * 64];
  }

  const int Lmax = tile_lengths(lens, n0, N, T, Ls);
  for (int i = threadIdx.x; i < 16 * LDG; i += 512) (&dg[0][0])[i] = 0.f;
  __syncthreads();

  // the rows no step writes
  for (int i = threadIdx.x; i < 16 * T * (G / 4); i += 512) {
    const int m = i / (T * (G / 4)), t = i / (G / 4) % T, k4 = i % (G / 4);
    if (n0 + m < N && t >= Ls[m])
      *(f32x4_t*)&dxproj[(((long)dir * N + n0 + m) * T + t) * G + 4 * k4] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  int Lr[4];
  long nr[4];
  float ds[4], dc[4], cs[4];
  const float* tp = tape + (((long)dir * gridDim.x + blockIdx.x) * T * 5 * 8 + w) * 256 + lane;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Lr[r] = Ls[4 * q + r];
    nr[r] = std::min(n0 + 4 * q + r, N - 1);
    ds[r] = dsent[nr[r] * 2 * H + dir * H + u];
    dc[r] = 0.f;
    cs[r] = Lmax > 0 ? tp[((long)(Lmax - 1) * 5 + 4) * TV + r * 64] : 0.f;
  }

  for (int s = Lmax - 1; s >= 0; --s) {
    // the step's tape values and dwords are requested first and consumed after the MFMA chain
    const float* ts = tp + (long)s * 5 * TV;
    float iv[4], fv[4], gv[4], ov[4], cp[4], dw[4];
    int tr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      iv[r] = ts[0 * TV + r * 64];
      fv[r] = ts[1 * TV + r * 64];
      gv[r] = ts[2 * TV + r * 64];
      ov[r] = ts[3 * TV + r * 64];
      cp[r] = s > 0 ? ts[-1 * TV + r * 64] : 0.f;  // c of step s - 1
      const bool run = s < Lr[r];
      tr[r] = !run ? 0 : dir == 0 ? s : Lr[r] - 1 - s;
      dw[r] = dwords[(nr[r] * 2 * H + dir * H + u) * Tout + std::min(tr[r], Tout - 1)];
    }

    // four partial sums over k (one per k-step of a read), added in a fixed order
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < KB / 4; ++s4) {
      const f32x4_t a = *(const f32x4_t*)&dg[col][16 * s4 + 4 * q];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bw[s4 * 4 + j], acc[j], 0, 0, 0);
    }
    __syncthreads();  // every wave has read the previous step's dgates

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool run = s < Lr[r];
      const float rec = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
      const float dh = (tr[r] < Tout ? dw[r] : 0.f) + (s == Lr[r] - 1 ? ds[r] : 0.f) + rec;
      const float tc = tanhf(cs[r]);
      const float dct = __fmaf_rn(dh * ov[r], 1.f - tc * tc, dc[r]);
      float da[4];
      da[0] = dct * gv[r] * iv[r] * (1.f - iv[r]);
      da[1] = dct * cp[r] * fv[r] * (1.f - fv[r]);
      da[2] = dct * iv[r] * (1.f - gv[r] * gv[r]);
      da[3] = dh * tc * ov[r] * (1.f - ov[r]);
      dc[r] = run ? dct * fv[r] : 0.f;
      cs[r] = cp[r];
      float* out = dxproj + (((long)dir * N + nr[r]) * T + tr[r]) * G + u;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        dg[4 * q + r][g * H + u] = run ? da[g] : 0.f;  // zero rows: the product needs no masking
        if (run) out[g * H] = da[g];
      }
    }
    __syncthreads();
  }
}

// out[r][e] = table[ids[r]][e] (* mask[r][e] * scale); ids clamped into the table
__global__ void embed_drop_kernel(const long* __restrict__ ids, long n, const float* __restrict__ table, int ntoken,
                                  int E, const uint8_t* __restrict__ mask, float scale, float* __restrict__ out) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n * E; e += (long)gridDim.x * blockDim.x) {
    const long r = e / E;
    const long tok = std::min<long>(std::max<long>(ids[r], 0), ntoken - 1);
    const float v = table[tok * E + (e % E)];
    out[e] = mask ? (mask[e] ? v * scale : 0.f) : v;
  }
}

// One workgroup per vocabulary row: the positions whose id is v, summed in index order.  The ids
// pass through LDS in chunks, and the test of a position is uniform across the workgroup.
constexpr int IDS_CHUNK = 2048;

__global__ __launch_bounds__(256) void embed_grad_kernel(const long* __restrict__ ids, long n,
                                                         const float* __restrict__ demb,
                                                         const uint8_t* __restrict__ mask, float scale, int ntoken,
                                                         int E, int accumulate, float* __restrict__ dtable) {
  __shared__ int toks[IDS_CHUNK];
  const int v = blockIdx.x;
  // columns threadIdx.x + 256 j, j < 4 (E <= 1024, checked by the host)
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (long p0 = 0; p0 < n; p0 += IDS_CHUNK) {
    const int cnt = (int)std::min<long>(IDS_CHUNK, n - p0);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += 256)
      toks[i] = (int)std::min<long>(std::max<long>(ids[p0 + i], 0), ntoken - 1);
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      if (toks[i] != v) continue;
      const long base = (p0 + i) * E;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = threadIdx.x + 256 * j;
        if (e < E) sum[j] += mask ? (mask[base + e] ? demb[base + e] * scale : 0.f) : demb[base + e];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = threadIdx.x + 256 * j;
    if (e < E) {
      float* o = dtable + (long)v * E + e;
      *o = accumulate ? *o + sum[j] : sum[j];
    }
  }
}

int check_shape(const char* what, int N, int T, int Hdim, int Tout) {
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

}  // namespace

extern "C" {

long eegan_lstm_train_workspace(int N, int T, int Hdim) {
  if (Hdim != H || N < 1 || T < 1) return 0;
  return 2L * ee_cdiv(N, 16) * T * 5 * TV * (long)sizeof(float);
}

int eegan_lstm_train_fwd(const float* xproj, const float* whh_packed, const long* lens, int N, int T, int Hdim,
                         int Tout, float* words, float* sent, float* tape, float* hprev, hipStream_t s) {
  if (int rc = check_shape("lstm_train_fwd", N, T, Hdim, Tout)) return rc;
  lstm_train_fwd_kernel<<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(xproj, whh_packed, lens, N, T, Tout, words, sent, tape,
                                                               hprev);
  return ee_check_launch("lstm_train_fwd");
}

int eegan_lstm_train_bwd(const float* dwords, const float* dsent, const float* whh_bwd_packed, const long* lens,
                         const float* tape, int N, int T, int Hdim, int Tout, float* dxproj, hipStream_t s) {
  if (int rc = check_shape("lstm_train_bwd", N, T, Hdim, Tout)) return rc;
  lstm_train_bwd_kernel<<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(dwords, dsent, whh_bwd_packed, lens, tape, N, T, Tout,
                                                               dxproj);
  return ee_check_launch("lstm_train_bwd");
}

int eegan_embedding_drop(const long* ids, long n, const float* table, int ntoken, int E, const uint8_t* mask,
                         float scale, float* out, hipStream_t s) {
  if (n < 1 || ntoken < 1 || E < 1) {
    ee_set_error("embedding_drop: n=%ld ntoken=%d E=%d", n, ntoken, E);
    return -22;
  }
  const int blocks = (int)std::max<long>(1, std::min<long>(4096, (n * E + 255) / 256));
  embed_drop_kernel<<<blocks, 256, 0, s>>>(ids, n, table, ntoken, E, mask, scale, out);
  return ee_check_launch("embedding_drop");
}

int eegan_embedding_grad(const long* ids, long n, const float* demb, const uint8_t* mask, float scale, int ntoken,
                         int E, int accumulate, float* dtable, hipStream_t s) {
  if (n < 1 || ntoken < 1 || E < 1 || E > 1024) {
    ee_set_error("embedding_grad: n=%ld ntoken=%d E=%d (E <= 1024)", n, ntoken, E);
    return -22;
  }
  embed_grad_kernel<<<ntoken, 256, 0, s>>>(ids, n, demb, mask, scale, ntoken, E, accumulate, dtable);
  return ee_check_launch("embedding_grad");
}

}  // extern "C"
