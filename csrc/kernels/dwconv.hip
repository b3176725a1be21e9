// Depthwise NHWC convolution (bf16 in / out, fp32 taps and accumulation) and its
// stride-2 transpose, for the K-UNet resamplers and the ConvNeXt 7x7 blocks.
//
//   y[b, oh, ow, c] = bias[c] + sum_{i<kh, j<kw} w[i, j, c] * xp[b, oh*s + i, ow*s + j, c]  (+ residual)
//
// xp is x padded by (pt, pl, pb, pr) with zeros or by reflection (F.pad
// "reflect": no edge repeat, pad < size); the padded tensor is never built, the
// index map below is applied where the input is read.  There is no reduction
// over channels, so no MFMA: a lane owns one 16-byte vector of 8 channels, a
// workgroup a DW_TH x DW_TW output tile of one block of <= 64 channels, a thread
// DW_R consecutive outputs of one tile row.  Sums run in tap order (i, then j)
// with one fma per tap, the residual is added in fp32, and the store rounds once.
//
// Two forward variants, picked by the caller (tools/dwconvbench.py times both):
//   halo:   the tile's input halo is staged in LDS once (16-byte vectors,
//           channels fastest across lanes), so an input element leaves L2 once
//           and not kh*kw times.  Rows have an odd pitch (in 128-byte pixels):
//           the 8 lane groups of a wave read 8 consecutive rows, which then fall
//           on alternating halves of the 64 banks (conflict-free ds_read_b128
//           at stride 1).
//   direct: every tap row is read straight from global memory (L1 / L2).
// The transposed op is a gather (no scatter, no atomics): an output pixel sums
// the taps whose parity matches it.
#include "common.h"

#define DW_TH 8        // output tile rows
#define DW_TW 16       // output tile columns
#define DW_R 4         // consecutive outputs per thread along W
#define DW_CV 8        // 16-byte channel vectors per workgroup (64 channels)
#define DW_THREADS 256 // DW_CV * DW_TH * (DW_TW / DW_R)
#define DW_KMAX 7

struct DwParams {
  const bf16_t* x;
  const float* w;      // [kh, kw, C] fp32
  const void* bias;    // [C] bf16 or fp32, or null
  const bf16_t* res;   // residual view or null
  bf16_t* out;
  int bias_f32;
  int B, H, W, C;      // unpadded input
  int xs, rs, os;      // pixel strides (elements) of x / residual / out
  int Ho, Wo;
  int kh, kw, stride;
  int pt, pl;          // top / left padding
  int Hp, Wp;          // padded input size (transposed op)
  int crop;            // conv_transpose2d "padding" (transposed op)
  int reflect;
};

// padded coordinate -> source coordinate, -1 where the padded tensor holds zero
// (also for coordinates beyond the padded tensor, which only ragged tiles touch)
__device__ __forceinline__ int dw_src(int p, int n, int reflect) {
  if (reflect) {
    if (p < 0) p = -p;
    else if (p >= n) p = 2 * (n - 1) - p;
  }
  return (p >= 0 && p < n) ? p : -1;
}

__device__ __forceinline__ void dw_bias(const DwParams& P, int c, float* a) {
  if (P.bias == nullptr) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = 0.f;
  } else if (P.bias_f32) {
    const float4 lo = *(const float4*)((const float*)P.bias + c), hi = *(const float4*)((const float*)P.bias + c + 4);
    a[0] = lo.x; a[1] = lo.y; a[2] = lo.z; a[3] = lo.w;
    a[4] = hi.x; a[5] = hi.y; a[6] = hi.z; a[7] = hi.w;
  } else {
    unpack8(*(const uint4*)((const bf16_t*)P.bias + c), a);
  }
}

__device__ __forceinline__ void dw_store(const DwParams& P, int b, int oh, int ow, int c, float* a) {
  const int64_t pix = ((int64_t)b * P.Ho + oh) * P.Wo + ow;
  if (P.res != nullptr) {
    float r[8];
    unpack8(*(const uint4*)(P.res + pix * P.rs + c), r);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += r[k];
  }
  *(uint4*)(P.out + pix * P.os + c) = pack8(a);
}

// KH = KW = S = 0: kernel size and stride read from the parameters
template <int KH, int KW, int S, bool HALO>
__global__ __launch_bounds__(DW_THREADS) void dwconv_kernel(const DwParams P) {
  extern __shared__ uint4 dw_smem[];
  const int kh = KH ? KH : P.kh, kw = KW ? KW : P.kw, s = S ? S : P.stride;
  const int tiles_w = (P.Wo + DW_TW - 1) / DW_TW;
  const int oh0 = ((int)blockIdx.x / tiles_w) * DW_TH, ow0 = ((int)blockIdx.x % tiles_w) * DW_TW;
  const int v0 = (int)blockIdx.y * DW_CV;        // first channel vector of the block
  const int nv = min(DW_CV, P.C / 8 - v0);       // vectors in it
  const int b = (int)blockIdx.z;
  const int tid = (int)threadIdx.x;
  float* wl = (float*)dw_smem;                   // taps [kh * kw][64] fp32
  uint4* hl = dw_smem + kh * kw * (DW_CV * 2);   // halo [iht][pitch][DW_CV]
  const int iht = (DW_TH - 1) * s + kh, iwt = (DW_TW - 1) * s + kw, pitch = iwt | 1;
  const int ih0 = oh0 * s - P.pt, iw0 = ow0 * s - P.pl;
  const bf16_t* xb = P.x + (int64_t)b * P.H * P.W * P.xs + v0 * 8;

  for (int e = tid; e < kh * kw * (DW_CV * 2); e += DW_THREADS) {  // float4 pieces, 16 per tap
    const int tap = e >> 4, q = e & 15;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (q * 4 < nv * 8) v = *(const float4*)(P.w + (int64_t)tap * P.C + v0 * 8 + q * 4);
    ((float4*)wl)[e] = v;
  }
  if (HALO) {
    for (int e = tid; e < iht * iwt * DW_CV; e += DW_THREADS) {
      const int cv = e & (DW_CV - 1), pix = e / DW_CV, hy = pix / iwt, hx = pix - hy * iwt;
      if (cv < nv) {
        const int ih = dw_src(ih0 + hy, P.H, P.reflect), iw = dw_src(iw0 + hx, P.W, P.reflect);
        uint4 v = {0u, 0u, 0u, 0u};
        if (ih >= 0 && iw >= 0) v = *(const uint4*)(xb + ((int64_t)ih * P.W + iw) * P.xs + cv * 8);
        hl[(hy * pitch + hx) * DW_CV + cv] = v;
      }
    }
  }
  __syncthreads();

  const int cv = tid & (DW_CV - 1), slot = tid / DW_CV;
  const int r = slot & (DW_TH - 1), cg = slot / DW_TH;  // a wave's 8 lane groups: 8 rows of one column group
  const int oh = oh0 + r, owb = ow0 + cg * DW_R;
  if (cv >= nv || oh >= P.Ho || owb >= P.Wo) return;    // the only barrier is behind us
  const int c = (v0 + cv) * 8;
  float acc[DW_R][8];
  dw_bias(P, c, acc[0]);
#pragma unroll
  for (int o = 1; o < DW_R; ++o)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[o][k] = acc[0][k];

  if constexpr (KH != 0) {
    // a tap row's weights and one input vector at a time in registers; input
    // column jx of the thread's span feeds output o through tap j = jx - o*S
    constexpr int NX = (DW_R - 1) * S + KW;
#pragma unroll 1  // one tap row in flight: unrolled, every row's loads are hoisted and the registers spill
    for (int i = 0; i < KH; ++i) {
      float wr[KW ? KW : 1][8];
#pragma unroll
      for (int j = 0; j < KW; ++j) {
        const float4 lo = *(const float4*)(wl + (i * KW + j) * 64 + cv * 8);
        const float4 hi = *(const float4*)(wl + (i * KW + j) * 64 + cv * 8 + 4);
        wr[j][0] = lo.x; wr[j][1] = lo.y; wr[j][2] = lo.z; wr[j][3] = lo.w;
        wr[j][4] = hi.x; wr[j][5] = hi.y; wr[j][6] = hi.z; wr[j][7] = hi.w;
      }
      const int ih = HALO ? 0 : dw_src(oh * S - P.pt + i, P.H, P.reflect);
#pragma unroll
      for (int jx = 0; jx < NX; ++jx) {
        uint4 v = {0u, 0u, 0u, 0u};
        if (HALO) {
          v = hl[((r * S + i) * pitch + cg * (DW_R * S) + jx) * DW_CV + cv];
        } else {
          const int iw = dw_src(owb * S - P.pl + jx, P.W, P.reflect);
          if (ih >= 0 && iw >= 0) v = *(const uint4*)(xb + ((int64_t)ih * P.W + iw) * P.xs + cv * 8);
        }
        float xf[8];
        unpack8(v, xf);
#pragma unroll
        for (int o = 0; o < DW_R; ++o) {
          const int j = jx - o * S;
          if (j >= 0 && j < KW) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[o][k] = __builtin_fmaf(wr[j][k], xf[k], acc[o][k]);
          }
        }
      }
    }
  } else {
    for (int o = 0; o < DW_R; ++o) {
      if (owb + o >= P.Wo) break;
      for (int i = 0; i < kh; ++i) {
        const int ih = HALO ? 0 : dw_src(oh * s - P.pt + i, P.H, P.reflect);
        for (int j = 0; j < kw; ++j) {
          uint4 v = {0u, 0u, 0u, 0u};
          if (HALO) {
            v = hl[((r * s + i) * pitch + (cg * DW_R + o) * s + j) * DW_CV + cv];
          } else {
            const int iw = dw_src((owb + o) * s - P.pl + j, P.W, P.reflect);
            if (ih >= 0 && iw >= 0) v = *(const uint4*)(xb + ((int64_t)ih * P.W + iw) * P.xs + cv * 8);
          }
          float xf[8];
          unpack8(v, xf);
          const float* wt = wl + (i * kw + j) * 64 + cv * 8;
          const float4 lo = *(const float4*)wt, hi = *(const float4*)(wt + 4);
          acc[o][0] = __builtin_fmaf(lo.x, xf[0], acc[o][0]); acc[o][1] = __builtin_fmaf(lo.y, xf[1], acc[o][1]);
          acc[o][2] = __builtin_fmaf(lo.z, xf[2], acc[o][2]); acc[o][3] = __builtin_fmaf(lo.w, xf[3], acc[o][3]);
          acc[o][4] = __builtin_fmaf(hi.x, xf[4], acc[o][4]); acc[o][5] = __builtin_fmaf(hi.y, xf[5], acc[o][5]);
          acc[o][6] = __builtin_fmaf(hi.z, xf[6], acc[o][6]); acc[o][7] = __builtin_fmaf(hi.w, xf[7], acc[o][7]);
        }
      }
    }
  }
#pragma unroll
  for (int o = 0; o < DW_R; ++o)
    if (owb + o < P.Wo) dw_store(P, b, oh, owb + o, c, acc[o]);
}

// y = conv_transpose2d(pad(x), w, stride 2, padding crop, groups C) as a gather:
// output row oh meets tap i iff (oh + crop - i) is even, reading padded input row
// (oh + crop - i) / 2; the same along W.  Taps come straight from global memory.
__global__ __launch_bounds__(DW_THREADS) void dwconv_t_kernel(const DwParams P) {
  const int tiles_w = (P.Wo + DW_TW - 1) / DW_TW;
  const int oh0 = ((int)blockIdx.x / tiles_w) * DW_TH, ow0 = ((int)blockIdx.x % tiles_w) * DW_TW;
  const int v0 = (int)blockIdx.y * DW_CV;
  const int nv = min(DW_CV, P.C / 8 - v0);
  const int b = (int)blockIdx.z;
  const int tid = (int)threadIdx.x;
  const int cv = tid & (DW_CV - 1), slot = tid / DW_CV;
  const int r = slot & (DW_TH - 1), cg = slot / DW_TH;
  const int oh = oh0 + r, owb = ow0 + cg * DW_R;
  if (cv >= nv || oh >= P.Ho || owb >= P.Wo) return;
  const int c = (v0 + cv) * 8;
  const bf16_t* xb = P.x + (int64_t)b * P.H * P.W * P.xs + c;
  float b0[8];
  dw_bias(P, c, b0);
  for (int o = 0; o < DW_R; ++o) {
    const int ow = owb + o;
    if (ow >= P.Wo) break;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = b0[k];
    for (int i = (oh + P.crop) & 1; i < P.kh; i += 2) {
      const int th = oh + P.crop - i;
      if (th < 0) break;
      if ((th >> 1) >= P.Hp) continue;
      const int ih = dw_src((th >> 1) - P.pt, P.H, P.reflect);
      if (ih < 0) continue;
      for (int j = (ow + P.crop) & 1; j < P.kw; j += 2) {
        const int tw = ow + P.crop - j;
        if (tw < 0) break;
        if ((tw >> 1) >= P.Wp) continue;
        const int iw = dw_src((tw >> 1) - P.pl, P.W, P.reflect);
        if (iw < 0) continue;
        float xf[8];
        unpack8(*(const uint4*)(xb + ((int64_t)ih * P.W + iw) * P.xs), xf);
        const float* wt = P.w + (int64_t)(i * P.kw + j) * P.C + c;
        const float4 lo = *(const float4*)wt, hi = *(const float4*)(wt + 4);
        acc[0] = __builtin_fmaf(lo.x, xf[0], acc[0]); acc[1] = __builtin_fmaf(lo.y, xf[1], acc[1]);
        acc[2] = __builtin_fmaf(lo.z, xf[2], acc[2]); acc[3] = __builtin_fmaf(lo.w, xf[3], acc[3]);
        acc[4] = __builtin_fmaf(hi.x, xf[4], acc[4]); acc[5] = __builtin_fmaf(hi.y, xf[5], acc[5]);
        acc[6] = __builtin_fmaf(hi.z, xf[6], acc[6]); acc[7] = __builtin_fmaf(hi.w, xf[7], acc[7]);
      }
    }
    dw_store(P, b, oh, ow, c, acc);
  }
}

// ---------------------------------------------------------------------------
static size_t dw_lds_bytes(int kh, int kw, int s, int halo) {
  const int iht = (DW_TH - 1) * s + kh, pitch = ((DW_TW - 1) * s + kw) | 1;
  return (size_t)kh * kw * 64 * sizeof(float) + (halo ? (size_t)iht * pitch * DW_CV * 16 : 0);
}

// the stride-2 halos pass the 64 KB a kernel gets without asking
template <typename K>
static hipError_t dw_allow_lds(K kernel) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)dw_lds_bytes(DW_KMAX, DW_KMAX, 2, 1));
}

static hipError_t dw_setup() {
  static hipError_t done = hipErrorNotReady;
  if (done != hipErrorNotReady) return done;
  hipError_t e = dw_allow_lds(dwconv_kernel<4, 4, 2, true>);
  if (e == hipSuccess) e = dw_allow_lds(dwconv_kernel<0, 0, 0, true>);
  return done = e;
}

static bool dw_geometry_ok(const DwParams& P) {
  return P.B >= 1 && P.B <= 65535 && P.C >= 8 && P.C % 8 == 0 && P.H >= 1 && P.W >= 1 && P.Ho >= 1 && P.Wo >= 1 &&
         P.kh >= 1 && P.kh <= DW_KMAX && P.kw >= 1 && P.kw <= DW_KMAX && P.xs % 8 == 0 && P.os % 8 == 0 &&
         (P.res == nullptr || P.rs % 8 == 0) && P.xs >= P.C && P.os >= P.C;
}

CSK_API int csk_dwconv_tile(int which) { return which == 0 ? DW_TH : which == 1 ? DW_TW : DW_CV * 8; }

// variant: 0 direct, 1 halo
CSK_API int csk_dwconv(const void* x, const void* w, const void* bias, int bias_f32, const void* res, void* out, int B,
                       int H, int W, int C, int xs, int rs, int os, int Ho, int Wo, int kh, int kw, int stride, int pt,
                       int pl, int reflect, int variant, hipStream_t stream) {
  DwParams P;
  P.x = (const bf16_t*)x; P.w = (const float*)w; P.bias = bias; P.res = (const bf16_t*)res; P.out = (bf16_t*)out;
  P.bias_f32 = bias_f32;
  P.B = B; P.H = H; P.W = W; P.C = C; P.xs = xs; P.rs = rs; P.os = os; P.Ho = Ho; P.Wo = Wo;
  P.kh = kh; P.kw = kw; P.stride = stride; P.pt = pt; P.pl = pl; P.Hp = 0; P.Wp = 0; P.crop = 0; P.reflect = reflect;
  if (!dw_geometry_ok(P) || (stride != 1 && stride != 2) || pt < 0 || pl < 0) return (int)hipErrorInvalidValue;
  const hipError_t e = dw_setup();
  if (e != hipSuccess) return (int)e;
  const dim3 grid(((Ho + DW_TH - 1) / DW_TH) * ((Wo + DW_TW - 1) / DW_TW), (C / 8 + DW_CV - 1) / DW_CV, B);
  const size_t lds = dw_lds_bytes(kh, kw, stride, variant);
#define DW_LAUNCH(KH_, KW_, S_)                                                                        \
  do {                                                                                                 \
    if (variant) hipLaunchKernelGGL((dwconv_kernel<KH_, KW_, S_, true>), grid, dim3(DW_THREADS), lds, stream, P);  \
    else hipLaunchKernelGGL((dwconv_kernel<KH_, KW_, S_, false>), grid, dim3(DW_THREADS), lds, stream, P);         \
  } while (0)
  if (kh == 7 && kw == 7 && stride == 1) DW_LAUNCH(7, 7, 1);
  else if (kh == 4 && kw == 4 && stride == 2) DW_LAUNCH(4, 4, 2);
  else DW_LAUNCH(0, 0, 0);
#undef DW_LAUNCH
  CSK_CHECK_LAUNCH();
}

CSK_API int csk_dwconv_t(const void* x, const void* w, const void* bias, int bias_f32, void* out, int B, int H, int W,
                         int C, int xs, int os, int Ho, int Wo, int kh, int kw, int pt, int pl, int Hp, int Wp,
                         int crop, int reflect, hipStream_t stream) {
  DwParams P;
  P.x = (const bf16_t*)x; P.w = (const float*)w; P.bias = bias; P.res = nullptr; P.out = (bf16_t*)out;
  P.bias_f32 = bias_f32;
  P.B = B; P.H = H; P.W = W; P.C = C; P.xs = xs; P.rs = 0; P.os = os; P.Ho = Ho; P.Wo = Wo;
  P.kh = kh; P.kw = kw; P.stride = 2; P.pt = pt; P.pl = pl; P.Hp = Hp; P.Wp = Wp; P.crop = crop; P.reflect = reflect;
  if (!dw_geometry_ok(P) || pt < 0 || pl < 0 || crop < 0 || Hp < H + pt || Wp < W + pl ||
      Ho != (Hp - 1) * 2 - 2 * crop + kh || Wo != (Wp - 1) * 2 - 2 * crop + kw)
    return (int)hipErrorInvalidValue;
  const dim3 grid(((Ho + DW_TH - 1) / DW_TH) * ((Wo + DW_TW - 1) / DW_TW), (C / 8 + DW_CV - 1) / DW_CV, B);
  hipLaunchKernelGGL(dwconv_t_kernel, grid, dim3(DW_THREADS), 0, stream, P);
  CSK_CHECK_LAUNCH();
}
