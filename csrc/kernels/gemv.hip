// Skinny-M GEMV for KV-cached decode: y[M, N] = act(norm?(x)[M, K] . W[N, K]^T + bias) + residual,
// M = 1 .. 8 rows, bf16 operands and output, fp32 sums; norm is LayerNorm or RMSNorm.
// Gated form (GLU = true): y = act(x' . Wg^T) * (x' . Wu^T) from two separate [N, K] matrices.
//
// A decode step reads every weight once and reuses nothing, so the kernel is a
// weight stream: a wave owns COLS output columns (rows of W), its lanes stride
// over K in 16-byte vectors that go straight from global memory to registers
// (no LDS, no MFMA: at M <= 8 an MFMA tile would be 87-99 % padding), 8 vectors
// per lane in flight before the first use and the next batch issued ahead of the
// current one's arithmetic.  Every weight vector is used for all M rows; the dot
// products end in a cross-lane wave reduce.
//
// The M input rows are read once per workgroup into LDS as fp32.  With
// gamma / beta given, the workgroup LayerNorms its copy there first: the mean,
// then the variance from the CENTRED values (the rows are on chip, so the second
// pass is free and there is no E[x^2] - mean^2 cancellation), and the normalised
// rows stay fp32: they are never rounded to bf16.  The first batch of weight
// loads is issued ahead of that prologue, so the LayerNorm runs in its shadow.
// RMSNorm (norm == GV_NORM_RMS) needs no mean: the sum of squares is taken in the
// pass that writes the rows, then one scale pass x * rstd * gamma.
//
// Epilogue order: bias, activation (gemm_common.h apply_act), residual, then ONE
// rounding at the store.  GEGLU pairs columns and is not supported.
//
// Gated form: a wave that owns COLS columns streams 2 * COLS weight rows (the
// gate row and the up row of each column) with UNR = 8 / (2 * COLS), so the same
// 8 vectors per lane are in flight; both sums finish in the same wave reduce and
// the storing lane computes act(gate) * up in fp32 and rounds once.  No bias, no
// residual.
//
// Grid: the largest (COLS, waves per workgroup) that still gives one workgroup
// per CU, so Bark's smallest matrix (N = 768) puts a wave on every CU.  The
// gated form uses the same rule: a column there costs two rows, so a workgroup
// moves twice the bytes, and LLaMA-7B's N = 11008 still gives 688 workgroups of
// (4, 4), 2.7 per CU (csk_gemv_plan reports the choice).
// W loads are non-temporal (every byte is used once per step; keeping 600 MB of
// weights out of the way of the activations and the KV cache) as a template
// parameter: csk_set_gemv_nt switches the instantiation for the A/B in
// tools/decodebench.py.
#include "gemm_common.h"  // apply_act and the ACT_* codes

typedef unsigned int gv_u4 __attribute__((ext_vector_type(4)));

#define GV_MAX_M 8
#define GV_LDS_FLOATS 32768  // MT * K fp32 input rows: 128 KB of the CU's 160 KB

#define GV_NORM_NONE 0
#define GV_NORM_LN 1
#define GV_NORM_RMS 2

struct GemvArgs {
  const bf16_t* x;      // [M][ldx]
  const bf16_t* w;      // [N][ldw], K-contiguous rows (gated form: the gate matrix)
  const bf16_t* w2;     // gated form: the up matrix [N][ldw2]; else null
  const bf16_t* bias;   // [N] or null
  const bf16_t* res;    // [M][ldr] or null
  bf16_t* y;            // [M][ldy]
  const bf16_t* gamma;  // [K]: LayerNorm / RMSNorm prologue (norm != GV_NORM_NONE)
  const bf16_t* beta;   // [K] or null (LayerNorm only)
  int M, N, K;
  int ldx, ldw, ldw2, ldr, ldy;
  int act, norm;
  float eps;
};

template <bool NT>
__device__ __forceinline__ gv_u4 gv_load_w(const bf16_t* p) {
  const gv_u4* q = (const gv_u4*)p;
  if (NT) return __builtin_nontemporal_load(q);
  return *q;
}

__device__ __forceinline__ void gv_unpack(const gv_u4& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

__device__ __forceinline__ void gv_lds_read8(const float* p, float* f) {
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
  f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}

__device__ __forceinline__ void gv_lds_write8(float* p, const float* f) {
  *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
  *(float4*)(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// COLS: output columns per wave; MT: input rows rounded up to 1 / 2 / 4 / 8
// (rows >= M are zeros in LDS and never stored); blockDim.x = 64 * waves;
// GLU: weight rows [0, COLS) of a wave are its gate rows, [COLS, 2 COLS) its up rows
template <int COLS, int MT, bool NT, bool GLU>
__global__ __launch_bounds__(256) void gemv_kernel(const GemvArgs a) {
  extern __shared__ float gv_x[];  // [MT][K] fp32 (normalised) input rows
  constexpr int OC = COLS;         // output columns per wave
  constexpr int R = GLU ? 2 * OC : OC;  // weight rows per wave
  constexpr int UNR = 8 / R;       // wave passes over K per batch: 8 weight vectors per lane in flight
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
  const int K = a.K;
  const int col0 = ((int)blockIdx.x * nw + wave) * OC;
  // columns past N read row N - 1 again and are dropped at the store: no wave leaves before the barrier
  const bf16_t* wr[R];
#pragma unroll
  for (int c = 0; c < R; ++c) {
    const int col = min(col0 + c % OC, a.N - 1);
    CSK_DCHECK(col >= 0 && col < a.N, 1, col, a.N);
    wr[c] = (c < OC ? a.w + (int64_t)col * a.ldw : a.w2 + (int64_t)col * a.ldw2) + lane * 8;
  }
  const int npass = (K + 511) >> 9;  // 64 lanes x 8 elements per wave pass
  const int nbatch = (npass + UNR - 1) / UNR;

  auto load_batch = [&](gv_u4 (&v)[UNR][R], int batch) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int k = ((batch * UNR + u) << 9) + lane * 8;
#pragma unroll
      for (int c = 0; c < R; ++c) {
        v[u][c] = gv_u4{0u, 0u, 0u, 0u};
        if (k < K) {  // K % 8 == 0: the whole vector is inside the row
          CSK_DCHECK(k + 8 <= K, 2, k, K);
          v[u][c] = gv_load_w<NT>(wr[c] + ((batch * UNR + u) << 9));
        }
      }
    }
  };

  gv_u4 cur[UNR][R];
  load_batch(cur, 0);  // in flight under the prologue below

  // input rows -> LDS fp32; wave w owns rows w, w + nw, ...: a lane reads back only what it wrote itself
  for (int m = wave; m < MT; m += nw) {
    float* xr = gv_x + m * K;
    float f[8];
    if (m >= a.M) {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = 0.f;
      for (int k = lane * 8; k < K; k += 512) gv_lds_write8(xr + k, f);
      continue;
    }
    const bf16_t* xg = a.x + (int64_t)m * a.ldx;
    float s = 0.f, ss = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
      CSK_DCHECK(k + 8 <= K, 3, k, K);
      unpack8(*(const uint4*)(xg + k), f);
      gv_lds_write8(xr + k, f);
      s += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(f[j], f[j], ss);
    }
    if (a.norm == GV_NORM_RMS) {
      const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)K + a.eps);
      for (int k = lane * 8; k < K; k += 512) {
        float g[8];
        unpack8(*(const uint4*)(a.gamma + k), g);
        gv_lds_read8(xr + k, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (f[j] * rstd) * g[j];
        gv_lds_write8(xr + k, f);
      }
    } else if (a.norm == GV_NORM_LN) {
      const float mean = wave_sum(s) / (float)K;
      float q = 0.f;
      for (int k = lane * 8; k < K; k += 512) {
        gv_lds_read8(xr + k, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = f[j] - mean;
          q = __builtin_fmaf(d, d, q);
        }
      }
      const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + a.eps);
      for (int k = lane * 8; k < K; k += 512) {
        float g[8], b[8];
        unpack8(*(const uint4*)(a.gamma + k), g);
        if (a.beta != nullptr) {
          unpack8(*(const uint4*)(a.beta + k), b);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] = 0.f;
        }
        gv_lds_read8(xr + k, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = __builtin_fmaf((f[j] - mean) * rstd, g[j], b[j]);
        gv_lds_write8(xr + k, f);
      }
    }
  }
  __syncthreads();

  float acc[R][MT];
#pragma unroll
  for (int c = 0; c < R; ++c)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[c][m] = 0.f;

  for (int b = 0; b < nbatch; ++b) {
    gv_u4 nxt[UNR][R];
    load_batch(nxt, b + 1);  // past the last batch every k >= K: zeros, no access
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int k = ((b * UNR + u) << 9) + lane * 8;
      if (k < K) {
        float wf[R][8];
#pragma unroll
        for (int c = 0; c < R; ++c) gv_unpack(cur[u][c], wf[c]);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          float xf[8];
          gv_lds_read8(gv_x + m * K + k, xf);
#pragma unroll
          for (int c = 0; c < R; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[c][m] = __builtin_fmaf(wf[c][j], xf[j], acc[c][m]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int c = 0; c < R; ++c) cur[u][c] = nxt[u][c];
  }

  // every lane ends with every sum; lane m * OC + c stores output (m, col0 + c)
  float v = 0.f, vu = 0.f;
#pragma unroll
  for (int c = 0; c < R; ++c)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float s = wave_sum(acc[c][m]);
      if (lane == m * OC + c % OC) {
        if (c < OC) v = s;
        else vu = s;
      }
    }
  const int m = lane / OC, col = col0 + lane % OC;
  if (lane < OC * MT && m < a.M && col < a.N) {
    if (GLU) {
      v = apply_act(a.act, v) * vu;
    } else {
      if (a.bias != nullptr) v += bf2f(a.bias[col]);
      v = apply_act(a.act, v);
      if (a.res != nullptr) v += bf2f(a.res[(int64_t)m * a.ldr + col]);
    }
    CSK_DCHECK(m >= 0 && m < a.M && col >= 0 && col < a.N, 4, col, a.N);
    a.y[(int64_t)m * a.ldy + col] = f2bf(v);
  }
}

// ---------------------------------------------------------------------------
static int g_gemv_nt = 1;

CSK_API int csk_set_gemv_nt(int v) {
  g_gemv_nt = v != 0;
  return 0;
}

CSK_API int csk_gemv_max_m() { return GV_MAX_M; }

static int gv_cu_count() {
  static int n = 0;
  if (n > 0) return n;
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
    v = 256;
  return n = v;
}

template <int COLS, int MT, bool NT, bool GLU>
static hipError_t gv_launch_one(const GemvArgs& a, int nw, hipStream_t stream) {
  // the M = 8, K = 4096 rows pass the 64 KB a kernel gets without asking
  static hipError_t attr = hipFuncSetAttribute((const void*)gemv_kernel<COLS, MT, NT, GLU>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, GV_LDS_FLOATS * 4);
  if (attr != hipSuccess) return attr;
  const int grid = (a.N + COLS * nw - 1) / (COLS * nw);
  hipLaunchKernelGGL((gemv_kernel<COLS, MT, NT, GLU>), dim3(grid), dim3(64 * nw), (size_t)MT * a.K * sizeof(float),
                     stream, a);
  return hipGetLastError();
}

template <int COLS, int MT, bool GLU>
static hipError_t gv_launch_nt(const GemvArgs& a, int nw, hipStream_t stream) {
  return g_gemv_nt ? gv_launch_one<COLS, MT, true, GLU>(a, nw, stream)
                   : gv_launch_one<COLS, MT, false, GLU>(a, nw, stream);
}

template <int COLS, bool GLU>
static hipError_t gv_launch_m(const GemvArgs& a, int mt, int nw, hipStream_t stream) {
  switch (mt) {
    case 1: return gv_launch_nt<COLS, 1, GLU>(a, nw, stream);
    case 2: return gv_launch_nt<COLS, 2, GLU>(a, nw, stream);
    case 4: return gv_launch_nt<COLS, 4, GLU>(a, nw, stream);
    default: return gv_launch_nt<COLS, 8, GLU>(a, nw, stream);
  }
}

template <bool GLU>
static hipError_t gv_launch_c(const GemvArgs& a, int cols, int mt, int nw, hipStream_t stream) {
  if (cols == 4) return gv_launch_m<4, GLU>(a, mt, nw, stream);
  if (cols == 2) return gv_launch_m<2, GLU>(a, mt, nw, stream);
  return gv_launch_m<1, GLU>(a, mt, nw, stream);
}

static bool gv_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the most columns per workgroup that still give every CU a workgroup
static void gv_plan(int N, int* cols, int* nw) {
  static const int plans[5][2] = {{4, 4}, {2, 4}, {1, 4}, {1, 2}, {1, 1}};  // (COLS, waves)
  const int cus = gv_cu_count();
  for (int i = 0; i < 5; ++i) {
    *cols = plans[i][0];
    *nw = plans[i][1];
    if ((N + *cols * *nw - 1) / (*cols * *nw) >= cus) break;
  }
}

// (columns per wave) * 16 + (waves per workgroup) of an N-column launch, plain or gated: for tests
CSK_API int csk_gemv_plan(int N) {
  int cols = 1, nw = 1;
  gv_plan(N < 1 ? 1 : N, &cols, &nw);
  return cols * 16 + nw;
}

// Graph-capturable: no allocation, no sync.  Anything outside the kernel's
// limits returns hipErrorInvalidValue (the Python side routes those shapes to
// its norm + gemm fallback before it gets here).  norm: GV_NORM_*; w2 != null
// selects the gated form y = act(x' w^T) * (x' w2^T), which takes no bias and no
// residual.
CSK_API int csk_gemv_ex(void* y, const void* x, const void* w, const void* w2, const void* bias, const void* res,
                        const void* gamma, const void* beta, int norm, int M, int N, int K, int ldx, int ldw,
                        int ldw2, int ldr, int ldy, int act, float eps, hipStream_t stream) {
  if (y == nullptr || x == nullptr || w == nullptr || M < 1 || M > GV_MAX_M || N < 1 || K < 8 || K % 8 != 0)
    return (int)hipErrorInvalidValue;
  if (ldw % 8 != 0 || ldw < K || !gv_aligned16(w) || !gv_aligned16(x) || (M > 1 && (ldx % 8 != 0 || ldx < K)))
    return (int)hipErrorInvalidValue;
  if (w2 != nullptr && (ldw2 % 8 != 0 || ldw2 < K || !gv_aligned16(w2) || bias != nullptr || res != nullptr))
    return (int)hipErrorInvalidValue;
  if (M > 1 && (ldy < N || (res != nullptr && ldr < N))) return (int)hipErrorInvalidValue;
  if (norm < GV_NORM_NONE || norm > GV_NORM_RMS || (norm != GV_NORM_NONE) != (gamma != nullptr) ||
      (norm != GV_NORM_LN && beta != nullptr) || !gv_aligned16(gamma) || !gv_aligned16(beta))
    return (int)hipErrorInvalidValue;
  if (act < 0 || act > ACT_GELU_TANH || act == ACT_GEGLU) return (int)hipErrorInvalidValue;
  const int mt = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8;
  if ((int64_t)mt * K > GV_LDS_FLOATS) return (int)hipErrorInvalidValue;
  GemvArgs a;
  a.x = (const bf16_t*)x; a.w = (const bf16_t*)w; a.w2 = (const bf16_t*)w2; a.bias = (const bf16_t*)bias;
  a.res = (const bf16_t*)res; a.y = (bf16_t*)y; a.gamma = (const bf16_t*)gamma; a.beta = (const bf16_t*)beta;
  a.M = M; a.N = N; a.K = K; a.ldx = ldx; a.ldw = ldw; a.ldw2 = ldw2; a.ldr = ldr; a.ldy = ldy; a.act = act;
  a.norm = norm; a.eps = eps;
  int cols = 1, nw = 1;
  gv_plan(N, &cols, &nw);
  return (int)(w2 != nullptr ? gv_launch_c<true>(a, cols, mt, nw, stream) : gv_launch_c<false>(a, cols, mt, nw, stream));
}

CSK_API int csk_gemv(void* y, const void* x, const void* w, const void* bias, const void* res, const void* gamma,
                     const void* beta, int M, int N, int K, int ldx, int ldw, int ldr, int ldy, int act, float eps,
                     hipStream_t stream) {
  if (gamma == nullptr && beta != nullptr) return (int)hipErrorInvalidValue;
  return csk_gemv_ex(y, x, w, nullptr, bias, res, gamma, beta, gamma != nullptr ? GV_NORM_LN : GV_NORM_NONE, M, N, K,
                     ldx, ldw, 0, ldr, ldy, act, eps, stream);
}

CSK_DEBUG_EXPORT(gemv)
