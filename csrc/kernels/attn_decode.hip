// Single-query split-KV attention for KV-cached decode, with the new token's
// K/V append fused in.
//
//   o[b, 0, h, :] = softmax(q[b, 0, h, :] . K[b, :n, h, :]^T * scale) V[b, :n, h, :],  n = clamp(*kv_len, 0, S)
//
// One query row per (b, h) fills 1 of 16 rows of an MFMA tile and leaves one
// workgroup per head walking up to S keys serially.  Here the grid is
// (nsplit, B * H) with nsplit = ceil(S / AD_SPLIT) fixed by the cache CAPACITY
// (the launch sits in a captured graph, so it cannot depend on kv_len): each
// workgroup scores its AD_SPLIT keys with K and V read straight to registers
// (D / 8 lanes per key, one 16-byte vector each, every load in flight before the
// first use), fp32 VALU dot products, a local softmax, and writes fp32
// (o[D], m, l) to a workspace.  Keys at or past n are never read.
//
// The combine runs in the same launch: a workgroup stores its partial
// write-through, drains the stores and takes a ticket from a per-(b, h) counter;
// the one that draws nsplit - 1 reads all partials back past its own caches and
// combines them in split order (so the result does not depend on who arrived
// last), stores the bf16 output and re-zeroes the counter.  Nobody waits on
// anybody: co-residency and dispatch order are irrelevant.  A split wholly past
// n publishes (0, -inf, 0).
//
// Append: with k_new / v_new given, the lanes that own key n - 1 take it from
// them instead of the cache and store it into the cache at that index.  No other
// workgroup reads or writes that row in this launch.
#include "common.h"

#define AD_SPLIT 64     // keys per workgroup
#define AD_THREADS 256

struct AdArgs {
  const bf16_t* q;
  bf16_t* kc;
  bf16_t* vc;
  const bf16_t* kn;  // new key / value [B, 1, H, D] or null
  const bf16_t* vn;
  bf16_t* o;
  float* ws;         // [B * H][nsplit][D + 2] fp32 partials
  unsigned* cnt;     // [B * H] arrival counters, zero between launches
  const int* kv_len;
  int64_t qs[2], ks[3], vs[3], kns[2], vns[2], os[2];  // element strides: (b, h) / (b, s, h)
  int B, H, S, nsplit;
  float scale;
};

template <int D>
__global__ __launch_bounds__(AD_THREADS) void attn_decode_kernel(const AdArgs a) {
  constexpr int LPK = D / 8;              // lanes per key (16-byte chunks of a row)
  constexpr int KPP = AD_THREADS / LPK;   // keys per workgroup pass
  constexpr int NP = AD_SPLIT / KPP;      // passes: 1 / 2 / 4 at D = 32 / 64 / 128
  constexpr int NW = AD_THREADS / 64;
  static_assert(NP >= 1 && NP * KPP == AD_SPLIT, "split / head dim");
  // one LDS object: [NW][D] output partials, [NW] maxima, [NW] sums, the "I am last" word
  __shared__ float sm[NW * D + 2 * NW + 1];
  float* sm_o = sm;
  float* sm_m = sm + NW * D;
  float* sm_l = sm_m + NW;
  float* sm_flag = sm_l + NW;

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = (int)blockIdx.x, bh = (int)blockIdx.y;
  const int b = bh / a.H, h = bh - b * a.H;
  const int n = min(max(*a.kv_len, 0), a.S);
  const int sub = tid % LPK, slot = tid / LPK;
  const float ninf = -__builtin_inff();

  float qf[8];
  unpack8(*(const uint4*)(a.q + b * a.qs[0] + h * a.qs[1] + sub * 8), qf);

  uint4 kr[NP], vr[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int idx = split * AD_SPLIT + p * KPP + slot;
    kr[p] = vr[p] = make_uint4(0u, 0u, 0u, 0u);
    if (idx < n) {
      CSK_DCHECK(idx >= 0 && idx < a.S, 1, idx, a.S);
      bf16_t* kp = a.kc + b * a.ks[0] + (int64_t)idx * a.ks[1] + h * a.ks[2] + sub * 8;
      bf16_t* vp = a.vc + b * a.vs[0] + (int64_t)idx * a.vs[1] + h * a.vs[2] + sub * 8;
      if (a.kn != nullptr && idx == n - 1) {
        kr[p] = *(const uint4*)(a.kn + b * a.kns[0] + h * a.kns[1] + sub * 8);
        vr[p] = *(const uint4*)(a.vn + b * a.vns[0] + h * a.vns[1] + sub * 8);
        *(uint4*)kp = kr[p];
        *(uint4*)vp = vr[p];
      } else {
        kr[p] = *(const uint4*)kp;
        vr[p] = *(const uint4*)vp;
      }
    }
  }

  float s[NP], m = ninf;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int idx = split * AD_SPLIT + p * KPP + slot;
    float kf[8], d = 0.f;
    unpack8(kr[p], kf);
#pragma unroll
    for (int j = 0; j < 8; ++j) d = __builtin_fmaf(qf[j], kf[j], d);
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) d += __shfl_xor(d, o, 64);  // the key's LPK lanes are one aligned group of a wave
    s[p] = idx < n ? d * a.scale : ninf;
    m = fmaxf(m, s[p]);
  }
  m = wave_max(m);
  if (lane == 0) sm_m[wave] = m;
  __syncthreads();
  m = sm_m[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) m = fmaxf(m, sm_m[w]);
  const float mm = m == ninf ? 0.f : m;  // a split with no live key: every exp below is exp(-inf) = 0

  float l = 0.f, of[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) of[j] = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float e = __expf(s[p] - mm);
    float vf[8];
    unpack8(vr[p], vf);
#pragma unroll
    for (int j = 0; j < 8; ++j) of[j] = __builtin_fmaf(e, vf[j], of[j]);
    if (sub == 0) l += e;  // one lane per key carries its weight into the sum
  }
  // over the wave's key slots: lanes with the same chunk
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1)
#pragma unroll
    for (int j = 0; j < 8; ++j) of[j] += __shfl_xor(of[j], o, 64);
  l = wave_sum(l);
  if (lane < LPK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sm_o[wave * D + lane * 8 + j] = of[j];
  }
  if (lane == 0) sm_l[wave] = l;
  __syncthreads();

  // this (b, h)'s partials as a buffer resource: stored write-through (sc1) and read back sc1, so the hand-off
  // needs no L2 write-back / invalidate (the fence-free form of gemm_common.h splitk_fixup)
  constexpr int PW = D + 2;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.ws + (int64_t)bh * a.nsplit * PW), 0, a.nsplit * PW * 4, 0x00020000);
  CSK_DCHECK(split >= 0 && split < a.nsplit, 2, split, a.nsplit);
  if (tid < D) {
    float v = sm_o[tid];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += sm_o[w * D + tid];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (split * PW + tid) * 4, 0, 16);
  }
  if (tid == 0) {
    float v = sm_l[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += sm_l[w];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), rs, (split * PW + D) * 4, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (split * PW + D + 1) * 4, 0, 16);
  }

  // publish: every wave drains its stores, then one ticket; the last arriver combines
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(a.cnt + bh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = old == (unsigned)(a.nsplit - 1);
    if (last) __hip_atomic_store(a.cnt + bh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
    *sm_flag = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (*sm_flag == 0.f || tid >= D) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (compiler order only: the loads below are sc1)

  // one pass in split order (the result does not depend on who arrived last), 8 splits' loads in flight at a time
  float gm = ninf, acc = 0.f, gl = 0.f;
  for (int i0 = 0; i0 < a.nsplit; i0 += 8) {
    float mi[8], li[8], oi[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int i = i0 + g;
      mi[g] = ninf;
      li[g] = oi[g] = 0.f;
      if (i < a.nsplit) {
        mi[g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (i * PW + D) * 4, 0, 16));
        li[g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (i * PW + D + 1) * 4, 0, 16));
        oi[g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (i * PW + tid) * 4, 0, 16));
      }
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (mi[g] == ninf) continue;  // a split with no live key
      if (mi[g] > gm) {
        const float sc = __expf(gm - mi[g]);  // gm = -inf: 0
        acc *= sc;
        gl *= sc;
        gm = mi[g];
      }
      const float w = __expf(mi[g] - gm);
      acc = __builtin_fmaf(w, oi[g], acc);
      gl = __builtin_fmaf(w, li[g], gl);
    }
  }
  a.o[b * a.os[0] + h * a.os[1] + tid] = f2bf(gl > 0.f ? acc / gl : 0.f);  // n = 0: zeros
}

CSK_API int csk_attn_decode_split() { return AD_SPLIT; }

static bool ad_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// st: element strides q (b, h), k (b, s, h), v (b, s, h), k_new (b, h), v_new (b, h), o (b, h).
// ws: fp32 [B * H * ceil(S / AD_SPLIT) * (D + 2)]; cnt: uint32 [B * H], zero on entry, zero on exit.
// Graph-capturable: no allocation, no sync.
CSK_API int csk_attention_decode(void* o, const void* q, void* kc, void* vc, const void* kn, const void* vn,
                                 const int64_t* st, int B, int H, int S, int D, float scale, const void* kv_len,
                                 void* ws, void* cnt, hipStream_t stream) {
  if (o == nullptr || q == nullptr || kc == nullptr || vc == nullptr || st == nullptr || kv_len == nullptr ||
      ws == nullptr || cnt == nullptr || (kn == nullptr) != (vn == nullptr))
    return (int)hipErrorInvalidValue;
  if ((D != 32 && D != 64 && D != 128) || B < 1 || H < 1 || S < 1 || (int64_t)B * H > 65535)
    return (int)hipErrorInvalidValue;
  if (!ad_aligned16(q) || !ad_aligned16(kc) || !ad_aligned16(vc) || !ad_aligned16(kn) || !ad_aligned16(vn))
    return (int)hipErrorInvalidValue;
  for (int i = 0; i < 12; ++i)  // every vector access is 16-byte aligned (o is stored by element)
    if (st[i] % 8 != 0 && !(kn == nullptr && i >= 8)) return (int)hipErrorInvalidValue;
  AdArgs a;
  a.q = (const bf16_t*)q; a.kc = (bf16_t*)kc; a.vc = (bf16_t*)vc; a.kn = (const bf16_t*)kn; a.vn = (const bf16_t*)vn;
  a.o = (bf16_t*)o; a.ws = (float*)ws; a.cnt = (unsigned*)cnt; a.kv_len = (const int*)kv_len;
  a.qs[0] = st[0]; a.qs[1] = st[1];
  a.ks[0] = st[2]; a.ks[1] = st[3]; a.ks[2] = st[4];
  a.vs[0] = st[5]; a.vs[1] = st[6]; a.vs[2] = st[7];
  a.kns[0] = st[8]; a.kns[1] = st[9]; a.vns[0] = st[10]; a.vns[1] = st[11];
  a.os[0] = st[12]; a.os[1] = st[13];
  a.B = B; a.H = H; a.S = S; a.nsplit = (S + AD_SPLIT - 1) / AD_SPLIT; a.scale = scale;
  const dim3 grid(a.nsplit, B * H);
  if (D == 32) hipLaunchKernelGGL(attn_decode_kernel<32>, grid, dim3(AD_THREADS), 0, stream, a);
  else if (D == 64) hipLaunchKernelGGL(attn_decode_kernel<64>, grid, dim3(AD_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(attn_decode_kernel<128>, grid, dim3(AD_THREADS), 0, stream, a);
  CSK_CHECK_LAUNCH();
}

CSK_DEBUG_EXPORT(attn_decode)
