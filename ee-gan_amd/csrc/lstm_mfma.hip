// The DAMSM text encoder's bi-LSTM recurrence (RNN_ENCODER, DAMSM.py:88-115) on
// v_mfma_f32_16x16x4_f32, H = 128: one forward kernel body for the sentence
// embeddings of R-precision (test.py:306-336) and for the trainable encoder's
// forward with a tape, and the back-propagation through time that reads the
// tape.  fp32 throughout, no atomics: every output element has one writer and
// every sum a fixed order, so two calls on the same inputs give the same bits.
//
// Work split, forward and backward: a workgroup of 8 waves owns 16 captions (a
// tile; the forward can own MT tiles) of one direction and wave w owns hidden
// units 16w..16w+15 of all four gates.  (caption 4q + r of the tile, unit
// u = 16w + lane%16) sits in lane (q, lane%16), register r of every accumulator
// tile, so the i/f/g/o pre-activations of one (caption, unit) meet in one lane:
// the cell arithmetic and the tape traffic are register-only, c never leaves
// registers.
//
// forward:  gates[16 x 4H] = h[16 x H] . W_hh^T; the wave's 128 x 64 slice of
//           W_hh^T is the resident B operand (128 VGPRs), h goes through a
//           padded double-buffered LDS array, one barrier per step.
//           x_t W_ih^T + b is a row of some table, requested before the MFMA
//           chain and added to the accumulators after it.
// backward: dh[16 x H] = dgates[16 x 4H] . W_hh; the wave's 512 x 16 slice of
//           W_hh is the resident B operand (128 VGPRs), dgates goes through one
//           padded LDS array, two barriers per step.
//
// tape [2][tiles][T steps][5: i f g o c][8 waves][4 r][64 lanes]: the
// accumulator order, so a wave stores and reloads each value as 256 B runs.
#include "common.h"
#include "rnn_tiles.h"
#include "../../include/eegan_hip.h"

namespace {

constexpr int H = 128;        // hidden units per direction (the DAMSM configs' only value)
constexpr int G = 4 * H;      // gate columns
constexpr int LDH = H + 4;    // h rows: 16 rows' float4 reads start 4 banks apart
constexpr int LDG = G + 4;    // dgates rows: 516 % 64 = 4, the same spread
constexpr int KS = H / 4;     // forward MFMA k-steps
constexpr int KB = G / 4;     // backward MFMA k-steps
constexpr int TV = 8 * 4 * 64;  // floats of one tape value of one (direction, tile, step)

// MFMA k-step s, lane quarter q reads k = 16 * (s / 4) + 4 * q + s % 4: the four steps 4j..4j+3 of
// a lane are four consecutive floats of h, so the A operand is one ds_read_b128 per four steps.  The
// host packs W_hh^T with the same map (functional.py: pack_whh_fwd).
//
// whh [2][8 waves][KS][4 gates][64 lanes], lens [N], sent [N][2H]; with TAPE also words [N][2H][Tout],
// tape (above, one tile per workgroup) and hprev [2][N*T][H]
template <int MT, class X, bool TAPE>
__global__ __launch_bounds__(512) void lstm_fwd_kernel(X xs, const float* __restrict__ whh,
                                                       const long* __restrict__ lens, int N, int T, int Tout,
                                                       float* __restrict__ sent, float* __restrict__ words,
                                                       float* __restrict__ tape, float* __restrict__ hprev) {
  static_assert(!TAPE || MT == 1, "the tape is laid out by 16-caption tiles, one per workgroup");
  constexpr int M = MT * 16;
  __shared__ __attribute__((aligned(16))) float hs[2][M][LDH];
  __shared__ int Ls[M];
  extern __shared__ int toks[];  // TokenTable's
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, col = lane & 15;
  const int dir = blockIdx.y;
  const int n0 = blockIdx.x * M;
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

  const int Lmax = tile_lengths(lens, n0, N, T, M, Ls);
  for (int i = threadIdx.x; i < 2 * M * LDH; i += 512) (&hs[0][0][0])[i] = 0.f;
  xs.template stage<M>(toks, n0, N, T);
  __syncthreads();

  float* tp = nullptr;
  if constexpr (TAPE) {
    // what no step writes: words and the h_prev rows past each caption's length
    for (int i = threadIdx.x; i < M * H * Tout; i += 512) {
      const int m = i / (H * Tout), k = i / Tout % H, t = i % Tout;
      if (n0 + m < N && t >= Ls[m]) words[((long)(n0 + m) * 2 * H + dir * H + k) * Tout + t] = 0.f;
    }
    for (int i = threadIdx.x; i < M * T * H; i += 512) {
      const int m = i / (T * H), t = i / H % T, k = i % H;
      if (n0 + m < N && t >= Ls[m]) hprev[(((long)dir * N + n0 + m) * T + t) * H + k] = 0.f;
    }
    tp = tape + (((long)dir * gridDim.x + blockIdx.x) * T * 5 * 8 + w) * 256 + lane;
  }

  // per register r of sub-tile mt: caption mt * 16 + 4q + r, its length and its state
  int Lr[MT][4];
  float c[MT][4], hv[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Lr[mt][r] = Ls[mt * 16 + 4 * q + r];
      c[mt][r] = hv[mt][r] = 0.f;
    }

  int cur = 0;
  for (int s = 0; s < Lmax; ++s) {
    // this step's x rows are requested first and added after the MFMA chain, which hides them
    f32x4_t x[MT][4], acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mt * 16 + 4 * q + r;
        const float* row = xs.template row<M>(toks, dir, n0, N, T, m, step_time(s, Lr[mt][r], dir)) + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) x[mt][g][r] = row[g * H];
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[mt][g] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      f32x4_t a[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *(const f32x4_t*)&hs[cur][mt * 16 + col][16 * s4 + 4 * q];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][j], bw[s4 * 4 + j][g], acc[mt][g], 0, 0, 0);
    }

    // accumulator (lane, r) = caption 4q + r of the tile, unit u, for every gate
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mt * 16 + 4 * q + r;
        const float ig = sigmoid_f(x[mt][0][r] + acc[mt][0][r]);
        const float fg = sigmoid_f(x[mt][1][r] + acc[mt][1][r]);
        const float gg = tanhf(x[mt][2][r] + acc[mt][2][r]);
        const float og = sigmoid_f(x[mt][3][r] + acc[mt][3][r]);
        const float cn = __fmaf_rn(fg, c[mt][r], ig * gg);
        const float hn = og * tanhf(cn);
        const int L = Lr[mt][r];
        const bool run = s < L;  // a select: the MFMAs need the whole wave
        if constexpr (TAPE) {
          const int t = step_time(s, L, dir);
          if (run) hprev[(((long)dir * N + n0 + m) * T + t) * H + u] = hv[mt][r];
          if (run && t < Tout) words[((long)(n0 + m) * 2 * H + dir * H + u) * Tout + t] = hn;
        }
        c[mt][r] = run ? cn : c[mt][r];
        hv[mt][r] = run ? hn : hv[mt][r];
        if constexpr (TAPE) {
          float* ts = tp + (long)s * 5 * TV + r * 64;
          ts[0 * TV] = ig;
          ts[1 * TV] = fg;
          ts[2 * TV] = gg;
          ts[3 * TV] = og;
          ts[4 * TV] = c[mt][r];
        }
        hs[cur ^ 1][m][u] = hv[mt][r];
      }
    __syncthreads();
    cur ^= 1;
  }

  // the last buffer holds every row's h at its own last step
  for (int i = threadIdx.x; i < M * H; i += 512) {
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

  const int Lmax = tile_lengths(lens, n0, N, T, 16, Ls);
  for (int i = threadIdx.x; i < 16 * LDG; i += 512) (&dg[0][0])[i] = 0.f;
  __syncthreads();

  // the rows no step writes
  for (int i = threadIdx.x; i < 16 * T * (G / 4); i += 512) {
    const int m = i / (T * (G / 4)), t = i / (G / 4) % T, k4 = i % (G / 4);
    if (n0 + m < N && t >= Ls[m])
      *(f32x4_t*)&dxproj[(((long)dir * N + n0 + m) * T + t) * G + 4 * k4] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // per register r: the caption's length and its (clamped) index
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
      tr[r] = step_time(s, Lr[r], dir);
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

}  // namespace

extern "C" {

int eegan_lstm_sent_batched(const float* xtab, const float* whh_packed, const long* ids, const long* lens, int N, int T,
                            int Hdim, int ntoken, float* sent, hipStream_t s) {
  if (Hdim != H) {
    ee_set_error("lstm_sent_batched: H=%d, only %d is built", Hdim, H);
    return -22;
  }
  if (N < 1 || T < 1 || T > 128 || ntoken < 1) {  // T: the tile's tokens sit in LDS
    ee_set_error("lstm_sent_batched: N=%d T=%d ntoken=%d", N, T, ntoken);
    return -22;
  }
  const TokenTable<G> xs{xtab, ids, ntoken};
  // one workgroup per CU is resident (its waves hold W_hh in registers): 16-caption tiles
  // while they all fit in one round, 32-caption tiles (half the weight loads) beyond that
  if (2 * ee_cdiv(N, 16) <= device_cus())
    lstm_fwd_kernel<1, TokenTable<G>, false><<<dim3(ee_cdiv(N, 16), 2), 512, 16 * T * sizeof(int), s>>>(
        xs, whh_packed, lens, N, T, 0, sent, nullptr, nullptr, nullptr);
  else
    lstm_fwd_kernel<2, TokenTable<G>, false><<<dim3(ee_cdiv(N, 32), 2), 512, 32 * T * sizeof(int), s>>>(
        xs, whh_packed, lens, N, T, 0, sent, nullptr, nullptr, nullptr);
  return ee_check_launch("lstm_sent_batched");
}

long eegan_lstm_train_workspace(int N, int T, int Hdim) {
  if (Hdim != H || N < 1 || T < 1) return 0;
  return 2L * ee_cdiv(N, 16) * T * 5 * TV * (long)sizeof(float);
}

int eegan_lstm_train_fwd(const float* xproj, const float* whh_packed, const long* lens, int N, int T, int Hdim,
                         int Tout, float* words, float* sent, float* tape, float* hprev, hipStream_t s) {
  if (int rc = check_train_shape("lstm_train_fwd", N, T, Hdim, Tout, H)) return rc;
  lstm_fwd_kernel<1, ProjRows<G>, true><<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(
      ProjRows<G>{xproj}, whh_packed, lens, N, T, Tout, sent, words, tape, hprev);
  return ee_check_launch("lstm_train_fwd");
}

int eegan_lstm_train_bwd(const float* dwords, const float* dsent, const float* whh_bwd_packed, const long* lens,
                         const float* tape, int N, int T, int Hdim, int Tout, float* dxproj, hipStream_t s) {
  if (int rc = check_train_shape("lstm_train_bwd", N, T, Hdim, Tout, H)) return rc;
  lstm_train_bwd_kernel<<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(dwords, dsent, whh_bwd_packed, lens, tape, N, T, Tout,
                                                               dxproj);
  return ee_check_launch("lstm_train_bwd");
}

}  // extern "C"
