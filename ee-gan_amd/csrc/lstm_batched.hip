// R-precision (test.py:306-336): sentence embeddings of thousands of short
// captions against one frozen bi-LSTM, and the cosine hit test.
//
// lstm_sent_kernel: eval-mode forward of RNN_ENCODER that keeps only the
// sentence embedding.  A workgroup of 8 waves owns MT*16 captions of one
// direction; wave w owns hidden units 16w..16w+15 of all four gates, with its
// 128 x 64 slice of W_hh^T resident in registers as the B operand of
// v_mfma_f32_16x16x4_f32 for the whole recurrence.  The i/f/g/o pre-activations
// of one (caption, unit) land in the same lane and register of the four
// accumulators, so the cell update is register-only; c never leaves registers
// and h goes through a padded, double-buffered LDS array, one barrier per step.
// x_t W_ih^T + b depends only on the token in eval mode: a row of a precomputed
// table, requested before the MFMA chain and added to the accumulators after it.
#include "common.h"
#include "../../include/eegan_hip.h"

namespace {

constexpr int H = 128;        // hidden units per direction (the DAMSM configs' only value)
constexpr int G = 4 * H;      // gate columns
constexpr int LDH = H + 4;    // LDS row stride: 16 rows' float4 reads start 4 banks apart
constexpr int KS = H / 4;     // MFMA k-steps

EE_DEV float sigmoid_f(float v) { return 1.f / (1.f + __expf(-v)); }

// MFMA k-step s, lane quarter q reads k = kidx(s, q): the four steps 4j..4j+3 of a
// lane are four consecutive floats of h, so the A operand is one ds_read_b128 per
// four steps.  The host packs W_hh with the same map (DAMSM.py: _sent_tables).
//   kidx(s, q) = 16 * (s / 4) + 4 * q + s % 4
//
// xtab [2][ntoken][4H], whh [2][8 waves][KS][4 gates][64 lanes], ids [N][T], lens [N], sent [N][2H]
template <int MT>
__global__ __launch_bounds__(512) void lstm_sent_kernel(const float* __restrict__ xtab, const float* __restrict__ whh,
                                                        const long* __restrict__ ids, const long* __restrict__ lens,
                                                        int N, int T, int ntoken, float* __restrict__ sent) {
  constexpr int M = MT * 16;
  __shared__ __attribute__((aligned(16))) float hs[2][M][LDH];
  __shared__ int Ls[M];
  extern __shared__ int toks[];  // [T][M]: the tile's tokens, clamped into the table
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

  // clamped lengths, 0 for the rows past N (they never step); the tile's maximum is uniform
  int Lmax = 0;
  for (int i = 0; i < M; ++i)
    if (n0 + i < N) Lmax = std::max(Lmax, (int)std::min<long>(std::max<long>(lens[n0 + i], 1), T));
  if (threadIdx.x < M) {
    const int n = n0 + threadIdx.x;
    Ls[threadIdx.x] = n < N ? (int)std::min<long>(std::max<long>(lens[n], 1), T) : 0;
  }
  for (int i = threadIdx.x; i < 2 * M * LDH; i += 512) (&hs[0][0][0])[i] = 0.f;
  for (int i = threadIdx.x; i < M * T; i += 512) {
    const int m = i / T, t = i - m * T;
    const long tok = n0 + m < N ? ids[(long)(n0 + m) * T + t] : 0;
    toks[t * M + m] = (int)std::min<long>(std::max<long>(tok, 0), ntoken - 1);
  }
  __syncthreads();

  const float* xt = xtab + (long)dir * ntoken * G + u;
  // x-projection rows of step s: xtab[dir][ids[n][t]] for running rows, zero for the rest
  auto fetch = [&](int s, f32x4_t (&x)[MT][4]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int L = Ls[mt * 16 + 4 * q + r];
        const bool run = s < L;
        const int t = !run ? 0 : dir == 0 ? s : L - 1 - s;
        const float* row = xt + (long)toks[t * M + mt * 16 + 4 * q + r] * G;
#pragma unroll
        for (int g = 0; g < 4; ++g) x[mt][g][r] = run ? row[g * H] : 0.f;
      }
  };

  float c[MT][4], hv[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[mt][r] = hv[mt][r] = 0.f;

  int cur = 0;
  for (int s = 0; s < Lmax; ++s) {
    // this step's table rows are requested first and added after the MFMA chain, which hides them
    f32x4_t x[MT][4], acc[MT][4];
    fetch(s, x);
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
        const float ig = sigmoid_f(x[mt][0][r] + acc[mt][0][r]);
        const float fg = sigmoid_f(x[mt][1][r] + acc[mt][1][r]);
        const float gg = tanhf(x[mt][2][r] + acc[mt][2][r]);
        const float og = sigmoid_f(x[mt][3][r] + acc[mt][3][r]);
        const float cn = __fmaf_rn(fg, c[mt][r], ig * gg);
        const float hn = og * tanhf(cn);
        const bool run = s < Ls[mt * 16 + 4 * q + r];  // a select: the MFMAs need the whole wave
        c[mt][r] = run ? cn : c[mt][r];
        hv[mt][r] = run ? hn : hv[mt][r];
        hs[cur ^ 1][mt * 16 + 4 * q + r][u] = hv[mt][r];
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

// One workgroup of RW waves per image: cosines of cnn_code[b] against [own[b]; cand[b][0..R-2]], hit
// iff no candidate scores strictly higher than the own sentence (torch.argmax == 0, first index on
// ties).  Lanes stride D and a row is reduced across the lanes of one wave; every wave scores the own
// sentence itself (the same bits in each) and then every RW-th candidate, and the verdicts meet in LDS.
constexpr int RW = 16;

EE_DEV float rprec_cos(const float* __restrict__ cv, const float* __restrict__ rv, int D, int lane, float cnorm) {
  float dot = 0.f, rr = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float x = rv[d];
    dot = __fmaf_rn(cv[d], x, dot);
    rr = __fmaf_rn(x, x, rr);
  }
  return wave_sum(dot) / fmaxf(cnorm * sqrtf(wave_sum(rr)), 1e-8f);
}

__global__ __launch_bounds__(64 * RW) void rprec_hits_kernel(const float* __restrict__ cnn,
                                                             const float* __restrict__ own,
                                                             const float* __restrict__ cand, int R, int D,
                                                             float* __restrict__ scores, int* __restrict__ hits) {
  __shared__ int beaten[RW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const float* cv = cnn + (long)b * D;
  float cc = 0.f;
  for (int d = lane; d < D; d += 64) cc = __fmaf_rn(cv[d], cv[d], cc);
  const float cnorm = sqrtf(wave_sum(cc));
  const float s0 = rprec_cos(cv, own + (long)b * D, D, lane, cnorm);
  if (scores && w == 0 && lane == 0) scores[(long)b * R] = s0;
  int lost = 0;
  for (int r = 1 + w; r < R; r += RW) {
    const float sc = rprec_cos(cv, cand + ((long)b * (R - 1) + (r - 1)) * D, D, lane, cnorm);
    lost |= sc > s0;
    if (scores && lane == 0) scores[(long)b * R + r] = sc;
  }
  if (lane == 0) beaten[w] = lost;
  __syncthreads();
  if (threadIdx.x == 0) {
    int any = 0;
    for (int i = 0; i < RW; ++i) any |= beaten[i];
    hits[b] = !any;
  }
}

int device_cus() {
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
  // one workgroup per CU is resident (its waves hold W_hh in registers): 16-caption tiles
  // while they all fit in one round, 32-caption tiles (half the weight loads) beyond that
  if (2 * ee_cdiv(N, 16) <= device_cus())
    lstm_sent_kernel<1><<<dim3(ee_cdiv(N, 16), 2), 512, 16 * T * sizeof(int), s>>>(xtab, whh_packed, ids, lens, N, T, ntoken, sent);
  else
    lstm_sent_kernel<2><<<dim3(ee_cdiv(N, 32), 2), 512, 32 * T * sizeof(int), s>>>(xtab, whh_packed, ids, lens, N, T, ntoken, sent);
  return ee_check_launch("lstm_sent_batched");
}

int eegan_rprec_hits(const float* cnn_code, const float* own, const float* cand, int B, int R, int D, float* scores,
                     int* hits, hipStream_t s) {
  if (B < 1 || R < 1 || D < 1) {
    ee_set_error("rprec_hits: B=%d R=%d D=%d", B, R, D);
    return -22;
  }
  rprec_hits_kernel<<<B, 64 * RW, 0, s>>>(cnn_code, own, cand, R, D, scores, hits);
  return ee_check_launch("rprec_hits");
}

}  // extern "C"
