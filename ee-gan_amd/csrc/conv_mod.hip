// Inference-only 3x3 conv with the affine_ssa modulation of its input fused in
// (gfx950, bf16 MFMA 16x16x32, fp32 accumulation).
//
//   z[n,p,c] = relu(x[n,p,c] * (a1[n,c] m[n,p] + a0[c]) + (b1[n,c] m[n,p] + b0[c]))
//   y[n,p,k] = res[n,p,k] + gamma * sum_{r,s,c} bf16(z[n, p + (r-1, s-1), c]) * W[k,r,s,c]
//
// z is SyncBN with RUNNING statistics + (gam*m + 1) * xhat + bet*m + ReLU
// (sync_batchnorm/batchnorm.py:48-53 in eval mode, models.py:69-86,113-122): a
// per-element map of x, so it is applied while the conv's B operand is staged
// and z never exists in HBM.  The training convs (conv.hip) move their operands
// global -> LDS by LDS-DMA and cannot transform them on the way; inference has no
// backward and nothing to save, so this kernel stages through registers.
//
// One workgroup (256 threads, 4 waves) owns 64 output channels x an 8 x 32 pixel
// tile of one image.  Per 32-channel input slice its threads load the 10 x 34
// source halo as 16-byte chunks (8 channels of one pixel) and the slice's
// 9 x 64 x 32 weights into VGPRs, apply the map in fp32 with the thread's mask
// values (its halo pixels are the same in every slice, so they stay in
// registers) and the sample's coefficient slice (LDS, one slice ahead), round to
// bf16 (RNE) and write ds_write_b128 into the slice image.  Halo positions
// outside the image are written as zero AFTER the map (the conv pads z, not x);
// channels >= C are never loaded (x's padding channels may hold anything).
// The loads of slice k+1 are issued before the 9 x 16 MFMAs per wave of slice k
// and written after them: a register-prefetch double buffer over ONE LDS image,
// two barriers per slice.
// LDS image as conv_halo3_kernel's: halo pixel h = (hy, hx)'s chunk q in slot
// h * 4 + (q ^ ((hx >> 1) & 2)), weights [tap][row][chunk ^ swz_b128(row >> 2)]:
// every tap's ds_read_b128 fragment read is conflict-free, a tap's shift is an
// immediate offset.  K order: slice-major, taps inside; no atomics; deterministic.
// Epilogue through LDS (fp32 tile, 16-B runs of 8 channels): res + gamma * acc,
// bf16 NHWC, pixels outside the image and channels >= K masked.
#include "common.h"
#include "../../include/eegan_hip.h"

namespace {

constexpr int TH = 8, TW = 32, TCO = 64, NT = 256, BK = 32;
constexpr int FI = TCO / 16, WROWS = TH / 4, CB = TW / 16, FJ = WROWS * CB;
constexpr int HW2 = TW + 2, HP = (TH + 2) * HW2;   // 340 halo pixels
constexpr int HOPS = (HP * 4 + NT - 1) / NT;       // 16-B halo chunks per thread (6; the last round is partial)
constexpr int WOPS = 9 * TCO * 4 / NT;             // 16-B weight chunks per thread: one per tap
constexpr int HBYTES = HP * 64, WBYTES = 9 * TCO * 64, CFLOATS = 4 * BK;
constexpr int STAGE = HBYTES + WBYTES + 2 * CFLOATS * 4;
constexpr int TPIX = TH * TW, NCK = TCO / 4, EPI = TPIX * TCO * 4;
constexpr int LDSB = STAGE > EPI ? STAGE : EPI;
// smallest conv grid (H * W) the fused kernel is dispatched at: it won at every generator shape, 4^2 included
constexpr long MODCONV_MIN_PIXELS = 1;
static_assert(WOPS * NT == 9 * TCO * 4 && WROWS * 4 == TH, "tile");

struct ModConvArgs {
  const bf16_t* x;
  const bf16_t* wp;
  const float* coef;   // [N][4][Cp]: a0, a1, b0, b1
  const float* mask;   // [N][H * W]
  const bf16_t* res;
  const float* gamma;
  bf16_t* y;
  int N, H, W, C, ldx, up2;   // (H, W): the conv's grid; x is physically (H >> up2) x (W >> up2)
  int K, ldy, ldres, res_up2;
  int Cgp, Kw, Cp;            // weight pack: per-tap channel run, row stride; coefficient row length
  int tiles_x, tiles_y;
};

EE_DEV int halo_swz(int hx) { return (hx >> 1) & 2; }
EE_DEV int swz_b128(int b) { return (0x1320 >> (b * 4)) & 3; }   // conv.hip: row-block permutation 0,2,3,1
EE_DEV bf16x8_t as_frag(uint4 v) { return __builtin_bit_cast(bf16x8_t, v); }

// a0 = inv_std, a1 = gam * inv_std, b0 = -mean * inv_std, b1 = bet - gam * mean * inv_std; zero for c >= C
__global__ void modconv_coef_kernel(const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                    const float* __restrict__ gam, const float* __restrict__ bet, int N, int C, int Cp,
                                    float* __restrict__ coef) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * Cp) return;
  const int n = i / Cp, c = i - n * Cp;
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
  if (c < C) {
    const float istd = 1.f / sqrtf(var[c] + eps), g = gam[n * C + c], mi = mean[c] * istd;
    a0 = istd;
    a1 = g * istd;
    b0 = -mi;
    b1 = bet[n * C + c] - g * mi;
  }
  float* o = coef + (long)n * 4 * Cp + c;
  o[0] = a0;
  o[Cp] = a1;
  o[2 * Cp] = b0;
  o[3 * Cp] = b1;
}

__global__ __launch_bounds__(NT, 2) void conv_mod3_kernel(ModConvArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[LDSB];
  char* const hl = lds;
  char* const wl = lds + HBYTES;
  float* const cl = reinterpret_cast<float*>(lds + HBYTES + WBYTES);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wj = __builtin_amdgcn_readfirstlane(tid >> 6);
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  const int n = b / a.tiles_y;
  const int oy0 = ty * TH, ox0 = tx * TW, co0 = blockIdx.y * TCO;
  const int nslice = (a.C + BK - 1) / BK;
  const int PH = a.H >> a.up2, PW = a.W >> a.up2;

  // this thread's halo chunks: logical channel chunk q of pixels (i * NT + tid) >> 2
  const int q = tid & 3;
  unsigned hoff[HOPS];
  int hdst[HOPS];
  float hm[HOPS];
  unsigned inimg = 0;
#pragma unroll
  for (int i = 0; i < HOPS; ++i) {
    const int L = i * NT + tid, h = L >> 2;
    const int hy = h / HW2, hx = h - hy * HW2;
    const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;   // conv-grid source pixel (pad 1)
    const bool ok = h < HP && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    hoff[i] = ok ? (unsigned)(((n * PH + (iy >> a.up2)) * PW + (ix >> a.up2)) * a.ldx + q * 8) : 0u;
    hm[i] = ok ? a.mask[(n * a.H + iy) * a.W + ix] : 0.f;   // the mask lives at the conv's resolution
    inimg |= (ok ? 1u : 0u) << i;
    hdst[i] = h * 64 + ((q ^ halo_swz(hx)) << 4);
  }
  // weight chunks: tap i, row tid >> 2, LDS slot tid & 3 holds channel chunk qw
  const int wrow = tid >> 2, qw = (tid & 3) ^ swz_b128((wrow >> 2) & 3);
  const bf16_t* const wsrc = a.wp + (long)(co0 + wrow) * a.Kw + qw * 8;   // rows are padded to 128: in range

  uint4 xr[HOPS], wr[WOPS];
  auto load = [&](int cs) {
    const bool cx = cs * BK + q * 8 < a.C, cw = cs * BK + qw * 8 < a.C;
#pragma unroll
    for (int i = 0; i < HOPS; ++i) {
      xr[i] = make_uint4(0, 0, 0, 0);
      if (cx && ((inimg >> i) & 1)) xr[i] = *reinterpret_cast<const uint4*>(a.x + hoff[i] + cs * BK);
    }
#pragma unroll
    for (int i = 0; i < WOPS; ++i) {
      wr[i] = make_uint4(0, 0, 0, 0);
      if (cw) wr[i] = *reinterpret_cast<const uint4*>(wsrc + i * a.Cgp + cs * BK);
    }
  };
  auto stage_coef = [&](int cs, int buf) {   // slice cs's four coefficient rows -> cl[buf]
    if (tid < CFLOATS && cs < nslice)
      cl[buf * CFLOATS + tid] = a.coef[((long)n * 4 + (tid >> 5)) * a.Cp + cs * BK + (tid & 31)];
  };
  auto store = [&](int cs) {   // transform slice cs (registers) -> LDS; coefficients from cl[cs & 1]
    const float4* cf = reinterpret_cast<const float4*>(cl + (cs & 1) * CFLOATS + q * 8);
    float k0[8], k1[8], k2[8], k3[8];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float4 v0 = cf[j], v1 = cf[8 + j], v2 = cf[16 + j], v3 = cf[24 + j];
      k0[4 * j] = v0.x, k0[4 * j + 1] = v0.y, k0[4 * j + 2] = v0.z, k0[4 * j + 3] = v0.w;
      k1[4 * j] = v1.x, k1[4 * j + 1] = v1.y, k1[4 * j + 2] = v1.z, k1[4 * j + 3] = v1.w;
      k2[4 * j] = v2.x, k2[4 * j + 1] = v2.y, k2[4 * j + 2] = v2.z, k2[4 * j + 3] = v2.w;
      k3[4 * j] = v3.x, k3[4 * j + 1] = v3.y, k3[4 * j + 2] = v3.z, k3[4 * j + 3] = v3.w;
    }
    const bool cx = cs * BK + q * 8 < a.C;
#pragma unroll
    for (int i = 0; i < HOPS; ++i) {
      if (i * NT + tid >= HP * 4) continue;
      uint4 o = make_uint4(0, 0, 0, 0);   // outside the image / past C: zero after the map
      if (cx && ((inimg >> i) & 1)) {
        const uint32_t w[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
        const float m = hm[i];
        uint32_t z[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s0 = __builtin_fmaf(k1[2 * e], m, k0[2 * e]), t0 = __builtin_fmaf(k3[2 * e], m, k2[2 * e]);
          const float s1 = __builtin_fmaf(k1[2 * e + 1], m, k0[2 * e + 1]),
                      t1 = __builtin_fmaf(k3[2 * e + 1], m, k2[2 * e + 1]);
          const float z0 = __builtin_fmaf(lo_f(w[e]), s0, t0), z1 = __builtin_fmaf(hi_f(w[e]), s1, t1);
          z[e] = pack2(z0 > 0.f ? z0 : 0.f, z1 > 0.f ? z1 : 0.f);
        }
        o = make_uint4(z[0], z[1], z[2], z[3]);
      }
      *reinterpret_cast<uint4*>(hl + hdst[i]) = o;
    }
#pragma unroll
    for (int i = 0; i < WOPS; ++i) *reinterpret_cast<uint4*>(wl + i * (TCO * 64) + tid * 16) = wr[i];
  };

  f32x4_t acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  // fragment addresses as conv_halo3_kernel: one base per tap column shift, immediates for the rest
  const int fwoff = fr * 64 + ((fq ^ swz_b128((fr >> 2) & 3)) << 4);
  int fhoff[3];
#pragma unroll
  for (int sx = 0; sx < 3; ++sx) fhoff[sx] = ((wj * WROWS * HW2 + fr + sx) << 6) + ((fq ^ halo_swz(fr + sx)) << 4);
  auto rd = [&](int t, bf16x8_t (&fa)[FI], bf16x8_t (&fb)[FJ]) {
    const int ta = t / 3, tb = t - ta * 3;
#pragma unroll
    for (int i = 0; i < FI; ++i) fa[i] = as_frag(*reinterpret_cast<const uint4*>(wl + fwoff + t * (TCO * 64) + i * 1024));
#pragma unroll
    for (int j = 0; j < FJ; ++j)
      fb[j] = as_frag(*reinterpret_cast<const uint4*>(hl + fhoff[tb] + (ta + j / CB) * (HW2 * 64) + (j % CB) * 1024));
  };

  stage_coef(0, 0);
  load(0);
  __syncthreads();
  stage_coef(1, 1);
  store(0);
  __syncthreads();
  for (int cs = 0; cs < nslice; ++cs) {
    const bool more = cs + 1 < nslice;
    if (more) load(cs + 1);   // in flight under this slice's MFMAs
    bf16x8_t fa[2][FI], fb[2][FJ];
    rd(0, fa[0], fb[0]);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      if (t + 1 < 9) rd(t + 1, fa[(t + 1) & 1], fb[(t + 1) & 1]);
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t & 1][i], fb[t & 1][j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();   // every wave is done with slice cs's image (the last slice: before the epilogue's tile)
    if (more) {
      stage_coef(cs + 2, cs & 1);   // cl[cs & 1] was last read when slice cs was stored
      store(cs + 1);
      __syncthreads();
    }
  }

  // epilogue: fp32 tile [pixel][16 chunks of 4 channels], chunk c of pixel p at c ^ (p & 15); every
  // thread then finishes 8 channels of one pixel.  The residual runs are loaded before the staging.
  constexpr int NIT = TPIX * (TCO / 8) / NT;
  uint4 rpre[NIT];
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int item = k * NT + tid, p = item / (TCO / 8), e = item % (TCO / 8);
    const int co = co0 + 8 * e, y = oy0 + p / TW, x = ox0 + p % TW;
    rpre[k] = make_uint4(0, 0, 0, 0);
    if (a.res && co < a.K && y < a.H && x < a.W) {
      const long rp = a.res_up2 ? ((long)n * (a.H >> 1) + (y >> 1)) * (a.W >> 1) + (x >> 1) : ((long)n * a.H + y) * a.W + x;
      rpre[k] = *reinterpret_cast<const uint4*>(a.res + rp * a.ldres + co);   // ldres % 8 == 0: inside the row
    }
  }
  float4* st = reinterpret_cast<float4*>(lds);
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    const int p = (wj * WROWS + j / CB) * TW + (j % CB) * 16 + fr;
#pragma unroll
    for (int i = 0; i < FI; ++i) {
      const int c = i * 4 + fq;
      st[p * NCK + (c ^ (p & 15))] = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
  __syncthreads();
  const float gam = (a.res && a.gamma) ? *a.gamma : 1.f;
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int item = k * NT + tid, p = item / (TCO / 8), e = item % (TCO / 8);
    const int co = co0 + 8 * e, y = oy0 + p / TW, x = ox0 + p % TW;
    if (co >= a.K || y >= a.H || x >= a.W) continue;
    const float4 lo = st[p * NCK + ((2 * e) ^ (p & 15))];
    const float4 hi = st[p * NCK + ((2 * e + 1) ^ (p & 15))];
    float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if (a.res) {
      const uint32_t rw[4] = {rpre[k].x, rpre[k].y, rpre[k].z, rpre[k].w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[2 * r] = __builtin_fmaf(gam, v[2 * r], lo_f(rw[r]));
        v[2 * r + 1] = __builtin_fmaf(gam, v[2 * r + 1], hi_f(rw[r]));
      }
    }
    bf16_t* dst = a.y + (((long)n * a.H + y) * a.W + x) * a.ldy + co;
    if (co + 8 > a.K) {   // the output row's last, partial chunk: nothing past K is written
      for (int r = 0; r < a.K - co; ++r) dst[r] = f2bf(v[r]);
      continue;
    }
    *reinterpret_cast<uint4*>(dst) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
  }
}

}  // namespace

extern "C" {

int eegan_modconv_coef(const float* running_mean, const float* running_var, float eps, const float* gam,
                       const float* bet, int N, int C, float* coef, hipStream_t stream) {
  if (N <= 0 || C <= 0) {
    ee_set_error("modconv_coef: N=%d C=%d", N, C);
    return -22;
  }
  const int Cp = ee_round_up(C, BK);
  ee_launch(modconv_coef_kernel, dim3(ee_cdiv((long)N * Cp, 256)), dim3(256), 0, stream, running_mean, running_var, eps,
            gam, bet, N, C, Cp, coef);
  return ee_check_launch("modconv_coef");
}

// The dispatch rule of SAGB_Block.infer, taken per shape from profiles/modconv_mi355x.txt: the fused
// launch where its median was not slower than eegan_bnmod_fwd + eegan_conv_fwd by more than the
// composition's own run-to-run spread.  EEGAN_CONV modconv=0: never; modconv=2: wherever it can run.
long eegan_modconv_use(const eegan_conv_desc* d) {
  const int k = ee_knob(getenv("EEGAN_CONV"), "modconv", 1);
  if (k == 0 || d->C <= 0 || d->C % 8 || d->R != 3 || d->S != 3 || d->stride != 1 || d->pad_h != 1 || d->pad_w != 1)
    return 0;
  if (k >= 2) return 1;
  return (long)d->H * d->W >= MODCONV_MIN_PIXELS;
}

int eegan_modconv_fwd(const eegan_conv_desc* d, const uint16_t* x, const uint16_t* wpack, const float* coef,
                      const float* mask, const uint16_t* res, int ldres, int res_up2, const float* gamma, uint16_t* y,
                      hipStream_t stream) {
  if (d->R != 3 || d->S != 3 || d->stride != 1 || d->pad_h != 1 || d->pad_w != 1 || d->Ho != d->H || d->Wo != d->W) {
    ee_set_error("modconv_fwd: 3x3 / stride 1 / pad 1 only (got %dx%d s%d p%d,%d, %dx%d -> %dx%d)", d->R, d->S,
                 d->stride, d->pad_h, d->pad_w, d->H, d->W, d->Ho, d->Wo);
    return -22;
  }
  if (d->C <= 0 || d->C % 8) {
    ee_set_error("modconv_fwd: C=%d must be a positive multiple of 8 (compose eegan_bnmod_fwd + eegan_conv_fwd)", d->C);
    return -22;
  }
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->K <= 0) return 0;
  if ((d->up2 || (res && res_up2)) && ((d->H | d->W) & 1)) {
    ee_set_error("modconv_fwd: a nearest-2x source needs an even grid (%dx%d)", d->H, d->W);
    return -22;
  }
  if (d->ldx < d->C || (d->ldx % 8) || ((uintptr_t)x & 15) || d->ldy < d->K || (d->ldy % 8) || ((uintptr_t)y & 15) ||
      (res && (ldres < d->K || (ldres % 8) || ((uintptr_t)res & 15)))) {
    ee_set_error("modconv_fwd: bf16 rows must be 16-byte aligned, channel strides multiples of 8 (ldx %d, ldy %d, ldres %d)",
                 d->ldx, d->ldy, ldres);
    return -22;
  }
  if (res && !gamma) {
    ee_set_error("modconv_fwd: residual without gamma");
    return -22;
  }
  // x / mask element offsets are 32-bit in the kernel
  const long HW = (long)d->H * d->W;
  if ((long)d->N * HW * std::max(d->ldx, 1) >= (1L << 31)) {
    ee_set_error("modconv_fwd: input of %ld elements exceeds the kernel's 32-bit offsets", (long)d->N * HW * d->ldx);
    return -22;
  }
  ModConvArgs a;
  a.x = x;
  a.wp = wpack;
  a.coef = coef;
  a.mask = mask;
  a.res = res;
  a.gamma = gamma;
  a.y = y;
  a.N = d->N, a.H = d->H, a.W = d->W, a.C = d->C, a.ldx = d->ldx, a.up2 = d->up2 ? 1 : 0;
  a.K = d->K, a.ldy = d->ldy, a.ldres = ldres, a.res_up2 = res_up2 ? 1 : 0;
  a.Cgp = d->C <= 8 ? 8 : ee_round_up(d->C, BK);   // the forward pack of eegan_conv_pack_weights
  a.Kw = ee_round_up(9 * a.Cgp, BK);
  a.Cp = ee_round_up(d->C, BK);
  a.tiles_x = ee_cdiv(d->W, TW);
  a.tiles_y = ee_cdiv(d->H, TH);
  const long tiles = (long)d->N * a.tiles_x * a.tiles_y;
  if (tiles >= (1L << 31)) {
    ee_set_error("modconv_fwd: %ld pixel tiles", tiles);
    return -22;
  }
  ee_launch(conv_mod3_kernel, dim3((unsigned)tiles, ee_cdiv(d->K, TCO)), dim3(NT), 0, stream, a);
  return ee_check_launch("conv_mod3");
}

}  // extern "C"
