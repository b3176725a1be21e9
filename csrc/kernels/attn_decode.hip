// Single-query split-KV attention for KV-cached decode, with the new token's
// K/V append, grouped K/V heads and the rotary embedding fused in.
//
//   o[b, 0, h, :] = softmax(q[b, 0, h, :] . K[b, :n, g, :]^T * scale) V[b, :n, g, :],  n = clamp(*kv_len, 0, S),
//   g = h / (H / Hkv): H / Hkv consecutive query heads share one K/V head.
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
// them, never from the cache.  With H > Hkv the H / Hkv workgroups of a group
// all own that index in the same split: every one of them reads k_new / v_new,
// and only the workgroup of the group's first query head (h % (H / Hkv) == 0)
// stores the row into the cache.  So in one launch cache row n - 1 of a K/V head
// has exactly one writer and no reader.
//
// RoPE (cos / sin given: fp32 [P][D / 2] tables, P >= S, row n - 1): rotate-half
// form, y[j] = x[j] cos[j] - x[j + D/2] sin[j], y[j + D/2] = x[j + D/2] cos[j] +
// x[j] sin[j].  The partner half of a lane's 8 elements is a second 16-byte load.
// The query is rotated in fp32 in every workgroup and used unrounded.  The new
// key is rotated in fp32 and rounded to bf16 once; that rounded value is both
// scored and stored, so the cache holds post-RoPE keys and a later step sees
// exactly what this step used.  v_new is not touched.
//
// D = 80 (OPT-2.7B): a row is ten 16-byte chunks.  A key keeps a 16-lane group
// (as at D = 128: 16 keys per pass, 4 passes) whose lanes 10..15 are idle: they
// load nothing, hold zeros in q and k, so add 0 to the dot product, and own no
// output chunk, which leaves the xor reductions over 1..8 and 16..32 as they
// are.  There is no RoPE at D = 80 (the launcher refuses the tables).
//
// Score bias (rb given: fp32 [H][PB], PB >= S): key idx of head h scores
// q . k * scale + rb[h][n - 1 - idx], a bias indexed by the key's distance to
// the query's own position n - 1 (T5's causal relative-position bias for the
// last query row, ALiBi).  It is added in fp32 after the lane reduce and before
// the running max; only distances [0, n) are read.
#include "common.h"

#define AD_SPLIT 64     // keys per workgroup
#define AD_THREADS 256

struct AdArgs {
  const bf16_t* q;
  bf16_t* kc;
  bf16_t* vc;
  const bf16_t* kn;  // new key / value [B, 1, Hkv, D] or null
  const bf16_t* vn;
  const float* cos;  // RoPE tables [P][D / 2] or null
  const float* sin;
  const float* rb;   // distance-indexed score bias [H][PB] or null
  bf16_t* o;
  float* ws;         // [B * H][nsplit][D + 2] fp32 partials
  unsigned* cnt;     // [B * H] arrival counters, zero between launches
  const int* kv_len;
  int64_t qs[2], ks[3], vs[3], kns[2], vns[2], os[2];  // element strides: (b, h) / (b, s, h)
  int B, H, S, nsplit;
  int rep;           // H / Hkv query heads per K/V head
  int PB;            // row length of rb
  float scale;
};

// x: this lane's 8 elements (chunk sub of a D-element row), xp: the same elements of the other half
// (chunk sub ^ (LPK / 2)); cs / sn: cos / sin at (sub % (LPK / 2)) * 8 of the position's table row
template <int LPK>
__device__ __forceinline__ void ad_rope8(float* x, const float* xp, const float* cs, const float* sn, int sub) {
  const float sg = sub < LPK / 2 ? -1.f : 1.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = __builtin_fmaf(sg * xp[j], sn[j], x[j] * cs[j]);
}

template <int D>
__global__ __launch_bounds__(AD_THREADS) void attn_decode_kernel(const AdArgs a) {
  constexpr int NCH = D / 8;              // 16-byte chunks of a row
  constexpr int LPK = NCH <= 4 ? 4 : NCH <= 8 ? 8 : 16;  // lanes per key: NCH rounded up to a power of two
  constexpr int KPP = AD_THREADS / LPK;   // keys per workgroup pass
  constexpr int NP = AD_SPLIT / KPP;      // passes: 1 / 2 / 4 / 4 at D = 32 / 64 / 80 / 128
  static_assert(D % 8 == 0 && NCH <= LPK && NCH > LPK / 2, "head dim");
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

  const int hk = h / a.rep;                    // the K/V head of this query head
  const bool writer = h - hk * a.rep == 0;     // the one workgroup of the group that stores the appended row
  const int psub = sub ^ (LPK / 2);            // the chunk that holds the rotation partners
  // D = 80: lanes 10..15 of a key's 16 own no chunk; they load nothing, add 0 to the dot product and hold no output
  const bool active = NCH == LPK || sub < NCH;

  float qf[8], cs[8], sn[8];
  unpack8(active ? *(const uint4*)(a.q + b * a.qs[0] + h * a.qs[1] + sub * 8) : make_uint4(0u, 0u, 0u, 0u), qf);
  if (NCH == LPK && a.cos != nullptr) {  // (the launcher takes no RoPE tables where NCH < LPK)
    const int pos = max(n - 1, 0);
    CSK_DCHECK(pos >= 0 && pos < a.S, 3, pos, a.S);
    const int64_t t = (int64_t)pos * (D / 2) + (sub % (LPK / 2)) * 8;
    const float4 c0 = *(const float4*)(a.cos + t), c1 = *(const float4*)(a.cos + t + 4);
    const float4 s0 = *(const float4*)(a.sin + t), s1 = *(const float4*)(a.sin + t + 4);
    cs[0] = c0.x; cs[1] = c0.y; cs[2] = c0.z; cs[3] = c0.w; cs[4] = c1.x; cs[5] = c1.y; cs[6] = c1.z; cs[7] = c1.w;
    sn[0] = s0.x; sn[1] = s0.y; sn[2] = s0.z; sn[3] = s0.w; sn[4] = s1.x; sn[5] = s1.y; sn[6] = s1.z; sn[7] = s1.w;
    float qp[8];
    unpack8(*(const uint4*)(a.q + b * a.qs[0] + h * a.qs[1] + psub * 8), qp);
    ad_rope8<LPK>(qf, qp, cs, sn, sub);
  }

  uint4 kr[NP], vr[NP];
  float rb[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int idx = split * AD_SPLIT + p * KPP + slot;
    kr[p] = vr[p] = make_uint4(0u, 0u, 0u, 0u);
    rb[p] = 0.f;
    if (a.rb != nullptr && idx < n) {  // the bias of distance n - 1 - idx, in [0, n) and so inside the row
      CSK_DCHECK(n - 1 - idx >= 0 && n - 1 - idx < a.PB, 4, n - 1 - idx, a.PB);
      rb[p] = a.rb[(int64_t)h * a.PB + (n - 1 - idx)];
    }
    if (idx < n && active) {
      CSK_DCHECK(idx >= 0 && idx < a.S, 1, idx, a.S);
      bf16_t* kp = a.kc + b * a.ks[0] + (int64_t)idx * a.ks[1] + hk * a.ks[2] + sub * 8;
      bf16_t* vp = a.vc + b * a.vs[0] + (int64_t)idx * a.vs[1] + hk * a.vs[2] + sub * 8;
      if (a.kn != nullptr && idx == n - 1) {
        const bf16_t* kn = a.kn + b * a.kns[0] + hk * a.kns[1];
        kr[p] = *(const uint4*)(kn + sub * 8);
        vr[p] = *(const uint4*)(a.vn + b * a.vns[0] + hk * a.vns[1] + sub * 8);
        if (NCH == LPK && a.cos != nullptr) {
          float kf[8], kq[8];
          unpack8(kr[p], kf);
          unpack8(*(const uint4*)(kn + psub * 8), kq);
          ad_rope8<LPK>(kf, kq, cs, sn, sub);
          kr[p] = pack8(kf);  // the one rounding: scored below and stored here
        }
        if (writer) {
          *(uint4*)kp = kr[p];
          *(uint4*)vp = vr[p];
        }
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
    s[p] = idx < n ? d * a.scale + rb[p] : ninf;  // (no table: + 0, the same value)
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
  if (lane < NCH) {
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
// Hkv: K/V heads of the caches and of k_new / v_new (H % Hkv == 0; their head strides in st are per K/V head).
// cos / sin: fp32 [P][D / 2] RoPE tables, P >= S, 16-byte aligned, or both null (D = 80 takes none).
// rel_bias: fp32 [H][PB] with PB >= S, 16-byte aligned, or null: key idx of head h scores
// q . k * scale + rel_bias[h][n - 1 - idx], n = clamp(*kv_len, 0, S).
CSK_API int csk_attention_decode_ex2(void* o, const void* q, void* kc, void* vc, const void* kn, const void* vn,
                                     const int64_t* st, int B, int H, int Hkv, int S, int D, float scale,
                                     const void* kv_len, void* ws, void* cnt, const void* cos, const void* sin, int P,
                                     const void* rel_bias, int PB, hipStream_t stream) {
  if (Hkv < 1 || H % Hkv != 0 || (cos == nullptr) != (sin == nullptr) || (cos != nullptr && P < S) ||
      !ad_aligned16(cos) || !ad_aligned16(sin))
    return (int)hipErrorInvalidValue;
  if ((cos != nullptr && D == 80) || (rel_bias != nullptr && PB < S) || !ad_aligned16(rel_bias))
    return (int)hipErrorInvalidValue;
  if (o == nullptr || q == nullptr || kc == nullptr || vc == nullptr || st == nullptr || kv_len == nullptr ||
      ws == nullptr || cnt == nullptr || (kn == nullptr) != (vn == nullptr))
    return (int)hipErrorInvalidValue;
  if ((D != 32 && D != 64 && D != 80 && D != 128) || B < 1 || H < 1 || S < 1 || (int64_t)B * H > 65535)
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
  a.cos = (const float*)cos; a.sin = (const float*)sin; a.rep = H / Hkv;
  a.rb = (const float*)rel_bias; a.PB = PB;
  a.B = B; a.H = H; a.S = S; a.nsplit = (S + AD_SPLIT - 1) / AD_SPLIT; a.scale = scale;
  const dim3 grid(a.nsplit, B * H);
  if (D == 32) hipLaunchKernelGGL(attn_decode_kernel<32>, grid, dim3(AD_THREADS), 0, stream, a);
  else if (D == 64) hipLaunchKernelGGL(attn_decode_kernel<64>, grid, dim3(AD_THREADS), 0, stream, a);
  else if (D == 80) hipLaunchKernelGGL(attn_decode_kernel<80>, grid, dim3(AD_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(attn_decode_kernel<128>, grid, dim3(AD_THREADS), 0, stream, a);
  CSK_CHECK_LAUNCH();
}

CSK_API int csk_attention_decode_ex(void* o, const void* q, void* kc, void* vc, const void* kn, const void* vn,
                                    const int64_t* st, int B, int H, int Hkv, int S, int D, float scale,
                                    const void* kv_len, void* ws, void* cnt, const void* cos, const void* sin, int P,
                                    hipStream_t stream) {
  return csk_attention_decode_ex2(o, q, kc, vc, kn, vn, st, B, H, Hkv, S, D, scale, kv_len, ws, cnt, cos, sin, P,
                                  nullptr, 0, stream);
}

CSK_API int csk_attention_decode(void* o, const void* q, void* kc, void* vc, const void* kn, const void* vn,
                                 const int64_t* st, int B, int H, int S, int D, float scale, const void* kv_len,
                                 void* ws, void* cnt, hipStream_t stream) {
  return csk_attention_decode_ex(o, q, kc, vc, kn, vn, st, B, H, H, S, D, scale, kv_len, ws, cnt, nullptr, nullptr, 0,
                                 stream);
}

CSK_DEBUG_EXPORT(attn_decode)
