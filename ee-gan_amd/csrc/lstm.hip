// Frozen DAMSM text encoder (RNN_ENCODER, DAMSM.py:30-115) in eval mode:
// embedding gather + bidirectional single-layer LSTM over each caption's own
// length.  Replaces nn.Embedding + pack_padded_sequence + nn.LSTM +
// pad_packed_sequence (DAMSM.py:91-105) without the host sync on
// cap_lens.tolist() (DAMSM.py:94): lengths are read on the device.
//
// Input projections x_t W_ih^T + b for all t are one fp32 GEMM per direction
// (eegan_gemm_f32); this file holds the gather and the recurrence, and the
// trainable encoder's masked gather and embedding gradient.  The fp32 MFMA
// recurrences for H = 128 are in lstm_mfma.hip.
#include "common.h"
#include "../../include/eegan_hip.h"

namespace {

__global__ void embed_kernel(const long* ids, long n, const float* table, int E, float* out) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n * E; e += (long)gridDim.x * blockDim.x) {
    const long r = e / E;
    out[e] = table[ids[r] * E + (e % E)];
  }
}

// The trainable encoder's gather (Fn.LstmTrainFn), with the dropout keep-mask fused in:
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

// Its gradient, no atomics.  One workgroup per vocabulary row: the positions whose id is v, summed in
// index order.  The ids pass through LDS in chunks, and the test of a position is uniform across the
// workgroup.
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

// grid (B, 2 directions), block 4H threads (one gate row each).
// xproj: [dir][B][T][4H] (bias included); whhT: [dir][H][4H] (transposed W_hh)
// words: [B][2H][Tout] (zero-filled by the caller); sent: [B][2H]
__global__ void lstm_seq_kernel(const float* xproj, const float* whhT, const long* lens, int B, int T, int H,
                                int Tout, float* words, float* sent) {
  extern __shared__ float sh[];
  float* h = sh;            // [H]
  float* gates = sh + H;    // [4H]
  const int b = blockIdx.x, dir = blockIdx.y, r = threadIdx.x;
  const int G = 4 * H;
  int L = (int)lens[b];
  if (L > T) L = T;
  if (r < H) h[r] = 0.f;
  float c = 0.f;
  __syncthreads();
  const float* W = whhT + (long)dir * H * G;
  const float* X = xproj + ((long)dir * B + b) * T * G;
  for (int s = 0; s < L; ++s) {
    const int t = dir == 0 ? s : L - 1 - s;
    float g = X[(long)t * G + r];
    for (int k = 0; k < H; ++k) g += W[(long)k * G + r] * h[k];
    gates[r] = g;
    __syncthreads();
    if (r < H) {
      const float ig = 1.f / (1.f + __expf(-gates[r]));
      const float fg = 1.f / (1.f + __expf(-gates[H + r]));
      const float gg = tanhf(gates[2 * H + r]);
      const float og = 1.f / (1.f + __expf(-gates[3 * H + r]));
      c = fg * c + ig * gg;
      const float hv = og * tanhf(c);
      h[r] = hv;
      if (t < Tout) words[((long)b * 2 * H + dir * H + r) * Tout + t] = hv;
    }
    __syncthreads();
  }
  if (r < H) sent[(long)b * 2 * H + dir * H + r] = h[r];
}

}  // namespace

extern "C" {

int eegan_embedding(const long* ids, long n, const float* table, int E, float* out, hipStream_t s) {
  const int blocks = (int)std::max<long>(1, std::min<long>(4096, (n * E + 255) / 256));
  embed_kernel<<<blocks, 256, 0, s>>>(ids, n, table, E, out);
  return ee_check_launch("embedding");
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

int eegan_lstm_bidir(const float* xproj, const float* whhT, const long* lens, int B, int T, int H, int Tout,
                     float* words, float* sent, hipStream_t s) {
  if (4 * H > 1024) {
    ee_set_error("lstm: 4H=%d > 1024", 4 * H);
    return -22;
  }
  (void)hipMemsetAsync(words, 0, (size_t)B * 2 * H * Tout * sizeof(float), s);
  lstm_seq_kernel<<<dim3(B, 2), 4 * H, 5 * H * sizeof(float), s>>>(xproj, whhT, lens, B, T, H, Tout, words, sent);
  return ee_check_launch("lstm_bidir");
}

}  // extern "C"
