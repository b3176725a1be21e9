// Fused attention forward with an additive score bias and per-sample key
// counts: O = softmax(Q K^T * scale + bias) V over each sample's first
// kv_lens[b] keys.  bf16 q/k/v/o as [B, S, H, D] strided views (D contiguous),
// fp32 bias logically [B, H, Sq, Skv] with the key dimension contiguous and
// element strides for b / h / q that may be 0 (broadcast), int32 kv_lens [B]
// read on the device (hipGraph-capturable).  The consumers are the text
// encoders: T5's relative-position bias (+ key padding), XLM-R's padded CFG
// batch, and padding-masked cross-attention — Skv is mostly 77, at most a few
// hundred, and B*H is 16..256 (batch, head) pairs.
//
// Structure = attn_fwd_kernel of attention.hip (swapped S^T = K Q^T on
// v_mfma_f32_16x16x32_bf16, one query column per lane, 4 consecutive keys per
// accumulator register group, P^T straight into the PV MFMA, V^T through
// ds_read_b64_tr_b16), with
//   * one query tile (16 rows) per wave and NW = 4 / 2 / 1 waves per workgroup,
//     so that 16..128 heads of 77 queries still spread over the chip;
//   * the lane's bias operand = four consecutive floats of one bias row per
//     register group (a 4-byte aligned 16-byte load: Skv = 77 rows are not
//     16-byte aligned), fetched one key block ahead;
//   * key j of sample b visible iff j < min(kv_lens[b], Skv) and, if causal,
//     j <= i + (Skv - Sq) with the TENSOR's Skv (padding-mask semantics, unlike
//     the KV-cache fill level `kv_len` of csk_attention);
//   * key blocks wholly past kv_lens[b] or above the causal diagonal skipped;
//   * the running max starts at a finite -1e30 and masked / -inf scores become
//     p = exp2(-inf) = 0, so a row with no visible key has l == 0 and writes
//     zeros, never NaN.
#include "common.h"

typedef __attribute__((address_space(3))) v4s lds_v4s;
typedef float v4f_u __attribute__((ext_vector_type(4), aligned(4)));

template <int CPR>
__device__ __forceinline__ int ab_off(int row, int chunk) {
  // element offset of 16-byte chunk `chunk` of row `row` in a [64][CPR*8] tile
  constexpr int MASK = CPR >= 16 ? 15 : CPR - 1;
  return row * (CPR * 8) + ((chunk ^ (row & MASK)) << 3);
}

struct AttnBiasArgs {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  long long sqb, sqs, sqh;  // element strides of q (b, s, h)
  long long skb, sks, skh;
  long long svb, svs, svh;
  long long sob, sos, soh;
  int B, H, Sq, Skv, D;
  float scale_log2;
  int causal;
  const float* bias;        // optional; [b][h][q][key], key contiguous
  long long sbb, sbh, sbq;  // element strides of bias (0 = broadcast)
  const int* kv_lens;       // optional; [B]
};

template <int DP, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bias_kernel(const AttnBiasArgs a) {
  constexpr int NT = 64 * NW;
  constexpr int CPR = DP / 8;        // 16B chunks per K/V row
  constexpr int KB = 64;             // keys per block
  constexpr int DS = DP / 32;        // k-steps of S = K Q^T over d
  constexpr int DT = DP / 16;        // O^T d-tiles
  constexpr int QROWS = 16 * NW;     // query rows per workgroup
  constexpr int TILE = KB * DP;      // elements per K or V tile
  constexpr int LPT = KB * CPR / NT; // 16B chunks per thread per tile
  constexpr float LOG2E = 1.4426950408889634f;
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * TILE];  // K0 V0 K1 V1

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nqb = (a.Sq + QROWS - 1) / QROWS;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = wg / nqb, qb = wg % nqb;
  const int b = bh / a.H, h = bh % a.H;
  const int q0 = qb * QROWS + wid * 16;
  const int qi = q0 + fr;              // this lane's query row
  const int coff = a.Skv - a.Sq;       // causal alignment: against the tensor's Skv
  const int klen = a.kv_lens ? max(0, min(a.Skv, a.kv_lens[b])) : a.Skv;

  const bf16_t* qp = a.q + b * a.sqb + h * a.sqh;
  const bf16_t* kp = a.k + b * a.skb + h * a.skh;
  const bf16_t* vp = a.v + b * a.svb + h * a.svh;
  // rows past Sq are computed (never stored): address them as the last row
  const float* bp = a.bias ? a.bias + b * a.sbb + h * a.sbh + (long long)min(qi, a.Sq - 1) * a.sbq : nullptr;

  // Q fragments (B operand): lane holds Q[qi][ds*32 + 8*fg .. +7]
  v8s qf[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    const int d = ds * 32 + 8 * fg;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (qi < a.Sq && d < a.D) v = *reinterpret_cast<const uint4*>(qp + qi * a.sqs + d);
    qf[ds] = __builtin_bit_cast(v8s, v);
  }

  v4f oacc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) oacc[i] = v4f{0.f, 0.f, 0.f, 0.f};
  float mrow = -1e30f, lrow = 0.f;

  // keys visible to ANY query row of this workgroup: [0, kv_end)
  int kv_end = klen;
  if (a.causal) kv_end = min(klen, min(a.Sq, (qb + 1) * QROWS) + coff);
  kv_end = max(kv_end, 0);
  const int nkb = (kv_end + KB - 1) / KB;

  uint4 rk[LPT], rv[LPT];
  auto load_kv = [&](int kb) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int id = tid + NT * i, row = id / CPR, c = id % CPR;
      const int key = kb * KB + row, d = c * 8;
      uint4 vk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (key < kv_end && d < a.D) {  // padding keys / values are never read: they need not be finite
        vk = *reinterpret_cast<const uint4*>(kp + key * a.sks + d);
        vv = *reinterpret_cast<const uint4*>(vp + key * a.svs + d);
      }
      rk[i] = vk;
      rv[i] = vv;
    }
  };
  auto store_kv = [&](int buf) {
    bf16_t* ks = smem + buf * 2 * TILE;
    bf16_t* vs = ks + TILE;
    CSK_DCHECK(buf >= 0 && buf < 2, 20, buf, 2);  // the 2-buffer K/V ring
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int id = tid + NT * i, row = id / CPR, c = id % CPR;
      CSK_DCHECK(ab_off<CPR>(row, c) + 8 <= TILE, 21, ab_off<CPR>(row, c), TILE);
      *reinterpret_cast<uint4*>(ks + ab_off<CPR>(row, c)) = rk[i];
      *reinterpret_cast<uint4*>(vs + ab_off<CPR>(row, c)) = rv[i];
    }
  };
  // bias of key block kb for this lane: bq[kt] = keys kb*64 + kt*16 + 4*fg + {0..3}
  // of the lane's row, pre-multiplied by log2(e) at use; keys >= kv_end stay 0
  // (their scores are masked) and are never addressed
  auto load_bias = [&](int kb, v4f* bq) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int key = kb * KB + kt * 16 + 4 * fg;
      v4f t = v4f{0.f, 0.f, 0.f, 0.f};
      if (bp) {
        if (key + 4 <= kv_end) {
          CSK_DCHECK(key + 4 <= a.Skv, 22, key, a.Skv);
          t = *reinterpret_cast<const v4f_u*>(bp + key);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key + r < kv_end) t[r] = bp[key + r];
        }
      }
      bq[kt] = t;
    }
  };

  v4f bcur[4], bnext[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) bcur[kt] = bnext[kt] = v4f{0.f, 0.f, 0.f, 0.f};
  if (nkb > 0) {
    load_bias(0, bcur);
    load_kv(0);
    store_kv(0);
  }
  __syncthreads();
  const float sl2 = a.scale_log2;
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    if (kb + 1 < nkb) {
      load_kv(kb + 1);
      load_bias(kb + 1, bnext);
    }
    const bf16_t* ks = smem + cur * 2 * TILE;
    const bf16_t* vs = ks + TILE;

    // ---- S^T = K Q^T : up to 4 key tiles; tiles wholly past kv_end are skipped ----
    const int kbase = kb * KB;
    const int ktn = min(4, (kv_end - kbase + 15) >> 4);
    v4f s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) s[kt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        if (kt >= ktn) continue;
        const v8s kf = *reinterpret_cast<const v8s*>(ks + ab_off<CPR>(kt * 16 + fr, ds * 4 + fg));
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ds], s[kt], 0, 0, 0);
      }
    }
    // ---- t = s * scale*log2e + bias*log2e, masks -> -inf, online softmax ----
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] = __builtin_fmaf(s[kt][r], sl2, bcur[kt][r] * LOG2E);
    if (a.causal || kbase + KB > kv_end) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kbase + kt * 16 + 4 * fg + r;
          if (key >= kv_end || (a.causal && key > qi + coff)) s[kt][r] = -INFINITY;
        }
    }
    float mx = vmax3(s[0][0], s[0][1], s[0][2]);
    mx = vmax3(mx, s[0][3], s[1][0]);
    mx = vmax3(mx, s[1][1], s[1][2]);
    mx = vmax3(mx, s[1][3], s[2][0]);
    mx = vmax3(mx, s[2][1], s[2][2]);
    mx = vmax3(mx, s[2][3], s[3][0]);
    mx = vmax3(mx, s[3][1], s[3][2]);
    mx = max_rowgroups(vmax3(mx, s[3][3], s[3][3]));
    // mrow >= -1e30 always: a block of -inf scores leaves it there, and
    // exp2(-inf - finite) = 0 (no inf - inf anywhere)
    const float mnew = fmaxf(mrow, mx);
    const float alpha = __builtin_amdgcn_exp2f(mrow - mnew);
    mrow = mnew;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - mnew);
    float l4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) l4[r] = vadd(vadd_t(s[0][r], s[1][r]), vadd_t(s[2][r], s[3][r]));
    lrow = lrow * alpha + vadd(vadd(l4[0], l4[1]), vadd(l4[2], l4[3]));
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oacc[dt] *= alpha;
    v8s pf[2];  // P^T fragments for the two 32-key PV k-steps
#pragma unroll
    for (int kp2 = 0; kp2 < 2; ++kp2) {
      u32 w0 = pack2(s[2 * kp2][0], s[2 * kp2][1]);
      u32 w1 = pack2(s[2 * kp2][2], s[2 * kp2][3]);
      u32 w2 = pack2(s[2 * kp2 + 1][0], s[2 * kp2 + 1][1]);
      u32 w3 = pack2(s[2 * kp2 + 1][2], s[2 * kp2 + 1][3]);
      pf[kp2] = __builtin_bit_cast(v8s, make_uint4(w0, w1, w2, w3));
    }
    // ---- O^T += V^T P^T ; V^T fragments via ds_read_b64_tr_b16 ----
#pragma unroll
    for (int kp2 = 0; kp2 < 2; ++kp2) {
      if (2 * kp2 >= ktn) continue;  // keys kp2*32 .. +31 all masked: P^T is zero there
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        // group fg reads rows (keys) kp2*32 + 4*fg + {0..3} and kp2*32 + 16 + 4*fg + {0..3},
        // lane 4q+p of the group addresses row q, columns dt*16 + 4p .. +3
        const int qq = fr >> 2, pp = fr & 3;
        const int col = dt * 16 + 4 * pp;
        const int r0 = kp2 * 32 + 4 * fg + qq, r1 = r0 + 16;
        const bf16_t* a0 = vs + ab_off<CPR>(r0, col >> 3) + (col & 7);
        const bf16_t* a1 = vs + ab_off<CPR>(r1, col >> 3) + (col & 7);
        v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(a0));
        v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(a1));
        v8s vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[kp2], oacc[dt], 0, 0, 0);
      }
    }
    if (kb + 1 < nkb) store_kv(cur ^ 1);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) bcur[kt] = bnext[kt];
    __syncthreads();
  }

  // ---- epilogue: reduce l over the 4 lane groups, normalise, store ----
  bf16_t* op = a.o + b * a.sob + h * a.soh;
  float l = lrow;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? 1.0f / l : 0.f;  // no visible key: zeros
  if (qi >= a.Sq) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + 4 * fg;
    if (d >= a.D) continue;
    uint2 w;
    w.x = pack2(oacc[dt][0] * inv, oacc[dt][1] * inv);
    w.y = pack2(oacc[dt][2] * inv, oacc[dt][3] * inv);
    *reinterpret_cast<uint2*>(op + qi * a.sos + d) = w;
  }
}

// Waves per workgroup: 0 = auto, or 1 / 2 / 4 (A/B knob of tools/attnbiasbench.py)
static int g_attn_bias_waves = 0;
CSK_API int csk_set_attn_bias_waves(int w) {
  if (w != 0 && w != 1 && w != 2 && w != 4) return (int)hipErrorInvalidValue;
  g_attn_bias_waves = w;
  return 0;
}

template <int DP, int NW>
static int launch_attn_bias(const AttnBiasArgs& a, long long wgs, hipStream_t s) {
  attn_bias_kernel<DP, NW><<<dim3((unsigned)wgs), 64 * NW, 0, s>>>(a);
  return (int)hipGetLastError();
}

template <int DP>
static int launch_attn_bias_d(const AttnBiasArgs& a, hipStream_t s) {
  const long long bh = (long long)a.B * a.H;
  auto wgs = [&](int nw) { return bh * ((a.Sq + 16 * nw - 1) / (16 * nw)); };
  int nw = g_attn_bias_waves;
  if (nw == 0) {
    // fewer waves per workgroup only while that makes MORE workgroups and the
    // grid does not yet cover the chip (256 CUs): T5-XXL (128 heads x 77
    // queries) 256 -> 384 workgroups; a decode step (Sq <= 16) keeps 4 waves,
    // whose idle ones still stage K / V
    nw = 4;
    if (wgs(4) < 256 && wgs(2) > wgs(4)) nw = 2;
    if (nw == 2 && wgs(2) < 256 && wgs(1) > wgs(2)) nw = 1;
  }
  const long long n = wgs(nw);
  if (n < 1 || n > 0x7fffffffll) return (int)hipErrorInvalidValue;
  if (nw == 1) return launch_attn_bias<DP, 1>(a, n, s);
  if (nw == 2) return launch_attn_bias<DP, 2>(a, n, s);
  return launch_attn_bias<DP, 4>(a, n, s);
}

// strides: q(b,s,h), k(b,s,h), v(b,s,h), o(b,s,h) in elements; bias_strides:
// (b, h, q) in elements of the fp32 bias (ignored when bias is null)
CSK_API int csk_attention_bias(void* o, const void* q, const void* k, const void* v, const long long* strides, int B,
                               int H, int Sq, int Skv, int D, float scale, int causal, const void* bias,
                               const long long* bias_strides, const void* kv_lens, hipStream_t stream) {
  if (D < 8 || D % 8 != 0 || D > 128 || B < 1 || H < 1 || Sq < 1 || Skv < 1) return (int)hipErrorInvalidValue;
  if (bias && !bias_strides) return (int)hipErrorInvalidValue;
  AttnBiasArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)o;
  a.sqb = strides[0]; a.sqs = strides[1]; a.sqh = strides[2];
  a.skb = strides[3]; a.sks = strides[4]; a.skh = strides[5];
  a.svb = strides[6]; a.svs = strides[7]; a.svh = strides[8];
  a.sob = strides[9]; a.sos = strides[10]; a.soh = strides[11];
  a.B = B; a.H = H; a.Sq = Sq; a.Skv = Skv; a.D = D;
  a.scale_log2 = scale * 1.4426950408889634f;
  a.causal = causal;
  a.bias = (const float*)bias;
  a.sbb = bias ? bias_strides[0] : 0;
  a.sbh = bias ? bias_strides[1] : 0;
  a.sbq = bias ? bias_strides[2] : 0;
  a.kv_lens = (const int*)kv_lens;
  if (D <= 64) return launch_attn_bias_d<64>(a, stream);
  return launch_attn_bias_d<128>(a, stream);
}

CSK_DEBUG_EXPORT(attn_bias)
