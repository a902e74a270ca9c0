// R-precision (test.py:306-336): the cosine hit test of each image code against
// its own sentence embedding and R-1 candidates (the embeddings come from
// eegan_lstm_sent_batched, lstm_mfma.hip).
#include "common.h"
#include "../../include/eegan_hip.h"

namespace {

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

}  // namespace

extern "C" {

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
