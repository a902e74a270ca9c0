// The DAMSM text encoder's bi-GRU recurrence (RNN_ENCODER with RNN_TYPE 'GRU', DAMSM.py:54-67) on
// v_mfma_f32_16x16x4_f32, H = 128: one forward kernel body for the sentence embeddings of
// R-precision, the frozen forward (words + sentence) and the trainable encoder's forward with a
// tape, and the back-propagation through time that reads the tape.  fp32 throughout, no atomics:
// every output element has one writer and every sum a fixed order, so two calls on the same inputs
// give the same bits.  torch.nn.GRU's cell:
//   r = s(x_r + W_hr h + b_hr)   z = s(x_z + W_hz h + b_hz)   n = tanh(x_n + r (W_hn h + b_hn))
//   h' = n + z (h - n)
//
// Work split as lstm_mfma.hip's: a workgroup of 8 waves owns 16 captions (a tile; the forward can
// own MT tiles) of one direction and wave w owns hidden units 16w..16w+15 of the three gates.
// (caption 4q + r of the tile, unit u = 16w + lane%16) sits in lane (q, lane%16), register r of
// every accumulator tile, so the r/z/n pre-activations of one (caption, unit) meet in one lane and
// the gate arithmetic is register-only.
//
// forward:  gates[16 x 3H] = h[16 x H] . W_hh^T; the wave's 128 x 48 slice of W_hh^T is the resident
//           B operand (96 VGPRs), h goes through a padded double-buffered LDS array, one barrier
//           per step.  The x row (b_ih, b_hr and b_hz folded in) is requested before the MFMA
//           chain and added after it; b_hn sits inside the r product and is one register per lane.
// backward: dh[16 x H] = [da_r da_z dhn][16 x 3H] . W_hh; the wave's 384 x 16 slice of W_hh is the
//           resident B operand (96 VGPRs), the hidden-side gate gradients go through one padded LDS
//           array, two barriers per step.
//
// tape [2][tiles][T steps][4: r z n hn][8 waves][4 r][64 lanes], hn = W_hn h + b_hn: the
// accumulator order, so a wave stores and reloads each value as 256 B runs.  The backward's
// h_{t-1} is read from hprev (row order, written for the weight-gradient GEMM anyway): 64 B runs
// that the MFMA chain hides, against 8 KB more tape per tile and step.
#include "common.h"
#include "rnn_tiles.h"
#include "../../include/eegan_hip.h"

namespace {

constexpr int H = 128;        // hidden units per direction (the DAMSM configs' only value)
constexpr int G = 3 * H;      // gate columns
constexpr int LDH = H + 4;    // h rows: 16 rows' float4 reads start 4 banks apart
constexpr int LDG = G + 4;    // gate-gradient rows: 388 % 64 = 4, the same spread
constexpr int KS = H / 4;     // forward MFMA k-steps
constexpr int KB = G / 4;     // backward MFMA k-steps
constexpr int TV = 8 * 4 * 64;  // floats of one tape value of one (direction, tile, step)
constexpr int NV = 4;           // tape values per step

enum { OUT_SENT = 0, OUT_WORDS = 1, OUT_TAPE = 2 };  // what the forward writes: each includes the one before

// MFMA k-step s, lane quarter q reads k = 16 * (s / 4) + 4 * q + s % 4 (lstm_mfma.hip's map): the A
// operand is one ds_read_b128 per four steps.  The host packs W_hh^T with the same map
// (functional.py: pack_whh_fwd with 3 gates).
//
// whh [2][8 waves][KS][3 gates][64 lanes], bhn [2][H], lens [N], sent [N][2H]; from OUT_WORDS also
// words [N][2H][Tout]; with OUT_TAPE also tape (above, one tile per workgroup) and hprev [2][N*T][H]
template <int MT, class X, int OUT>
__global__ __launch_bounds__(512) void gru_fwd_kernel(X xs, const float* __restrict__ whh,
                                                      const float* __restrict__ bhn, const long* __restrict__ lens,
                                                      int N, int T, int Tout, float* __restrict__ sent,
                                                      float* __restrict__ words, float* __restrict__ tape,
                                                      float* __restrict__ hprev) {
  static_assert(OUT != OUT_TAPE || MT == 1, "the tape is laid out by 16-caption tiles, one per workgroup");
  constexpr int M = MT * 16;
  __shared__ __attribute__((aligned(16))) float hs[2][M][LDH];
  __shared__ int Ls[M];
  extern __shared__ int toks[];  // TokenTable's
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, col = lane & 15;
  const int dir = blockIdx.y;
  const int n0 = blockIdx.x * M;
  const int u = 16 * w + col;  // this lane's hidden unit

  // the wave's W_hh^T slice and the lane's b_hn, once
  float bw[KS][3];
  {
    const float* wp = whh + ((long)(dir * 8 + w) * KS * 3) * 64 + lane;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int g = 0; g < 3; ++g) bw[s][g] = wp[(s * 3 + g) * 64];
  }
  const float bn = bhn[dir * H + u];

  const int Lmax = tile_lengths(lens, n0, N, T, M, Ls);
  for (int i = threadIdx.x; i < 2 * M * LDH; i += 512) (&hs[0][0][0])[i] = 0.f;
  xs.template stage<M>(toks, n0, N, T);
  __syncthreads();

  // what no step writes: words and the h_prev rows past each caption's length
  if constexpr (OUT >= OUT_WORDS)
    for (int i = threadIdx.x; i < M * H * Tout; i += 512) {
      const int m = i / (H * Tout), k = i / Tout % H, t = i % Tout;
      if (n0 + m < N && t >= Ls[m]) words[((long)(n0 + m) * 2 * H + dir * H + k) * Tout + t] = 0.f;
    }
  float* tp = nullptr;
  if constexpr (OUT == OUT_TAPE) {
    for (int i = threadIdx.x; i < M * T * H; i += 512) {
      const int m = i / (T * H), t = i / H % T, k = i % H;
      if (n0 + m < N && t >= Ls[m]) hprev[(((long)dir * N + n0 + m) * T + t) * H + k] = 0.f;
    }
    tp = tape + (((long)dir * gridDim.x + blockIdx.x) * T * NV * 8 + w) * 256 + lane;
  }

  // per register r of sub-tile mt: caption mt * 16 + 4q + r, its length and its state
  int Lr[MT][4];
  float hv[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Lr[mt][r] = Ls[mt * 16 + 4 * q + r];
      hv[mt][r] = 0.f;
    }

  int cur = 0;
  for (int s = 0; s < Lmax; ++s) {
    // this step's x rows are requested first and added after the MFMA chain, which hides them
    f32x4_t x[MT][3], acc[MT][3];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mt * 16 + 4 * q + r;
        const float* row = xs.template row<M>(toks, dir, n0, N, T, m, step_time(s, Lr[mt][r], dir)) + u;
#pragma unroll
        for (int g = 0; g < 3; ++g) x[mt][g][r] = row[g * H];
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[mt][g] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      f32x4_t a[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *(const f32x4_t*)&hs[cur][mt * 16 + col][16 * s4 + 4 * q];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 3; ++g)
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
        const float rg = sigmoid_f(x[mt][0][r] + acc[mt][0][r]);
        const float zg = sigmoid_f(x[mt][1][r] + acc[mt][1][r]);
        const float hg = acc[mt][2][r] + bn;
        const float ng = tanhf(__fmaf_rn(rg, hg, x[mt][2][r]));
        const float hn = __fmaf_rn(zg, hv[mt][r] - ng, ng);
        const int L = Lr[mt][r];
        const bool run = s < L;  // a select: the MFMAs need the whole wave
        if constexpr (OUT >= OUT_WORDS) {
          const int t = step_time(s, L, dir);
          if constexpr (OUT == OUT_TAPE)
            if (run) hprev[(((long)dir * N + n0 + m) * T + t) * H + u] = hv[mt][r];
          if (run && t < Tout) words[((long)(n0 + m) * 2 * H + dir * H + u) * Tout + t] = hn;
        }
        hv[mt][r] = run ? hn : hv[mt][r];
        if constexpr (OUT == OUT_TAPE) {
          float* ts = tp + (long)s * NV * TV + r * 64;
          ts[0 * TV] = rg;
          ts[1 * TV] = zg;
          ts[2 * TV] = ng;
          ts[3 * TV] = hg;
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

// With dh' = dwords + dsent (at the caption's last step) + the recurrent part:
//   dn = dh' (1 - z)   dz = dh' (h - n)   da_n = dn (1 - n^2)   da_r = da_n hn r (1 - r)
//   da_z = dz z (1 - z)   dhn = da_n r   dh = dh' z + [da_r da_z dhn] . W_hh
// The input side's gate gradients are [da_r da_z da_n], the hidden side's [da_r da_z dhn]: they
// differ in the n third only, so the hidden side's reaches HBM as that third alone.
//
// dwords [N][2H][Tout], dsent [N][2H], wbk [2][8 waves][KB][64 lanes] (W_hh, not transposed), lens [N],
// tape and hprev as written by the forward; dxproj [2][N*T][3H], dhn [2][N*T][H]
__global__ __launch_bounds__(512) void gru_train_bwd_kernel(const float* __restrict__ dwords,
                                                            const float* __restrict__ dsent,
                                                            const float* __restrict__ wbk,
                                                            const long* __restrict__ lens,
                                                            const float* __restrict__ tape,
                                                            const float* __restrict__ hprev, int N, int T, int Tout,
                                                            float* __restrict__ dxproj, float* __restrict__ dhn) {
  __shared__ __attribute__((aligned(16))) float dg[16][LDG];
  __shared__ int Ls[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, col = lane & 15;
  const int dir = blockIdx.y;
  const int n0 = blockIdx.x * 16;
  const int u = 16 * w + col;

  // the wave's 384 x 16 slice of W_hh, once
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
  for (int i = threadIdx.x; i < 16 * T * (H / 4); i += 512) {
    const int m = i / (T * (H / 4)), t = i / (H / 4) % T, k4 = i % (H / 4);
    if (n0 + m < N && t >= Ls[m])
      *(f32x4_t*)&dhn[(((long)dir * N + n0 + m) * T + t) * H + 4 * k4] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // per register r: the caption's length, its (clamped) index and dh' z of the step above
  int Lr[4];
  long nr[4];
  float ds[4], dhz[4];
  const float* tp = tape + (((long)dir * gridDim.x + blockIdx.x) * T * NV * 8 + w) * 256 + lane;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Lr[r] = Ls[4 * q + r];
    nr[r] = std::min(n0 + 4 * q + r, N - 1);
    ds[r] = dsent[nr[r] * 2 * H + dir * H + u];
    dhz[r] = 0.f;
  }

  for (int s = Lmax - 1; s >= 0; --s) {
    // the step's tape values, h_{t-1} and dwords are requested first and consumed after the MFMA chain
    const float* ts = tp + (long)s * NV * TV;
    float rv[4], zv[4], nv[4], hg[4], hp[4], dw[4];
    int tr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      rv[r] = ts[0 * TV + r * 64];
      zv[r] = ts[1 * TV + r * 64];
      nv[r] = ts[2 * TV + r * 64];
      hg[r] = ts[3 * TV + r * 64];
      tr[r] = step_time(s, Lr[r], dir);
      hp[r] = hprev[(((long)dir * N + nr[r]) * T + tr[r]) * H + u];
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
    __syncthreads();  // every wave has read the previous step's gate gradients

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool run = s < Lr[r];
      const float rec = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
      const float dh = (tr[r] < Tout ? dw[r] : 0.f) + (s == Lr[r] - 1 ? ds[r] : 0.f) + (rec + dhz[r]);
      const float dan = dh * (1.f - zv[r]) * (1.f - nv[r] * nv[r]);
      float da[4];  // r, z, n of the input side; n of the hidden side
      da[0] = dan * hg[r] * rv[r] * (1.f - rv[r]);
      da[1] = dh * (hp[r] - nv[r]) * zv[r] * (1.f - zv[r]);
      da[2] = dan;
      da[3] = dan * rv[r];
      dhz[r] = run ? dh * zv[r] : 0.f;
      const long row = ((long)dir * N + nr[r]) * T + tr[r];
      float* out = dxproj + row * G + u;
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        dg[4 * q + r][g * H + u] = run ? da[g == 2 ? 3 : g] : 0.f;  // zero rows: the product needs no masking
        if (run) out[g * H] = da[g];
      }
      if (run) dhn[row * H + u] = da[3];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int eegan_gru_sent_batched(const float* xtab, const float* whh_packed, const float* bhn, const long* ids,
                           const long* lens, int N, int T, int Hdim, int ntoken, float* sent, hipStream_t s) {
  if (Hdim != H) {
    ee_set_error("gru_sent_batched: H=%d, only %d is built", Hdim, H);
    return -22;
  }
  if (N < 1 || T < 1 || T > 128 || ntoken < 1) {  // T: the tile's tokens sit in LDS
    ee_set_error("gru_sent_batched: N=%d T=%d ntoken=%d", N, T, ntoken);
    return -22;
  }
  const TokenTable<G> xs{xtab, ids, ntoken};
  // A step is a serial chain of 96 MFMAs per 16 captions and one workgroup per CU is resident
  // either way, so 16-caption tiles while they all fit in one round (half the chain per step);
  // 32-caption tiles (half the rounds and weight loads) beyond that
  if (2 * ee_cdiv(N, 16) <= device_cus())
    gru_fwd_kernel<1, TokenTable<G>, OUT_SENT><<<dim3(ee_cdiv(N, 16), 2), 512, 16 * T * sizeof(int), s>>>(
        xs, whh_packed, bhn, lens, N, T, 0, sent, nullptr, nullptr, nullptr);
  else
    gru_fwd_kernel<2, TokenTable<G>, OUT_SENT><<<dim3(ee_cdiv(N, 32), 2), 512, 32 * T * sizeof(int), s>>>(
        xs, whh_packed, bhn, lens, N, T, 0, sent, nullptr, nullptr, nullptr);
  return ee_check_launch("gru_sent_batched");
}

int eegan_gru_fwd(const float* xproj, const float* whh_packed, const float* bhn, const long* lens, int N, int T,
                  int Hdim, int Tout, float* words, float* sent, hipStream_t s) {
  if (int rc = check_train_shape("gru_fwd", N, T, Hdim, Tout, H)) return rc;
  gru_fwd_kernel<1, ProjRows<G>, OUT_WORDS><<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(
      ProjRows<G>{xproj}, whh_packed, bhn, lens, N, T, Tout, sent, words, nullptr, nullptr);
  return ee_check_launch("gru_fwd");
}

long eegan_gru_train_workspace(int N, int T, int Hdim) {
  if (Hdim != H || N < 1 || T < 1) return 0;
  return 2L * ee_cdiv(N, 16) * T * NV * TV * (long)sizeof(float);
}

int eegan_gru_train_fwd(const float* xproj, const float* whh_packed, const float* bhn, const long* lens, int N, int T,
                        int Hdim, int Tout, float* words, float* sent, float* tape, float* hprev, hipStream_t s) {
  if (int rc = check_train_shape("gru_train_fwd", N, T, Hdim, Tout, H)) return rc;
  gru_fwd_kernel<1, ProjRows<G>, OUT_TAPE><<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(
      ProjRows<G>{xproj}, whh_packed, bhn, lens, N, T, Tout, sent, words, tape, hprev);
  return ee_check_launch("gru_train_fwd");
}

int eegan_gru_train_bwd(const float* dwords, const float* dsent, const float* whh_bwd_packed, const long* lens,
                        const float* tape, const float* hprev, int N, int T, int Hdim, int Tout, float* dxproj,
                        float* dhn, hipStream_t s) {
  if (int rc = check_train_shape("gru_train_bwd", N, T, Hdim, Tout, H)) return rc;
  gru_train_bwd_kernel<<<dim3(ee_cdiv(N, 16), 2), 512, 0, s>>>(dwords, dsent, whh_bwd_packed, lens, tape, hprev, N, T,
                                                              Tout, dxproj, dhn);
  return ee_check_launch("gru_train_bwd");
}

}  // extern "C"
