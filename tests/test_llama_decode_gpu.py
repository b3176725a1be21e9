"""The LLaMA decode kernels on the GPU: the GEMV's RMSNorm prologue and its
gated two-matrix form (csrc/kernels/gemv.hip), the decode attention's rotary
embedding and grouped K/V heads (attn_decode.hip), the five-launch layer inside
a replayed hipGraph, and ``LlamaLM.decode_step`` wired to them.  Conventions of
tests/test_decode_gpu.py: strided views of wider tensors, a sentinel-filled
output buffer, ``DECODE_STATS`` proving that the kernel ran, float64 CPU
references from the bf16 tensors.

GEMV with ``rms=``.  ``assert_bf16_close(y, ref, S, K)`` requires
|y - ref| <= 2^-8 |ref| + (K + 4) 2^-22 S of every element with

    S = T |W|^T + |bias| + |residual|,   T = |x| rstd |gamma|.

The kernel sums x^2 in fp32: K non-negative terms, so the sum is off by at most
(K + 7) 2^-24 relative whatever the order (8 fused multiply-adds per lane pass,
then the wave reduce); mean + eps, the square root and the reciprocal add three
roundings and halve the relative error of the sum, so rstd carries at most
(K / 2 + 7) 2^-24.  A normalised element (x rstd) gamma adds two roundings:
(K / 2 + 9) 2^-24 T.  The fp32 dot product over these elements adds
(K + 4) 2^-24 T |W|^T.  Together below (1.5 K + 13) 2^-24, inside the helper's
(K + 4) 2^-22 = (4 K + 16) 2^-24 unit.

Gated form, y = silu(g) u with g, u the two dot products.  With Sg, Su their
absolute-value twins the fp32 error of silu(g) u is at most
(K + 4) 2^-22 (1.1 Sg |u| + |silu(g)| Su) (1.1: sup |silu'| = 1.0998 rounded
up) plus the activation's own error.  common.h states no bound for silu_f
(__expf and v_rcp_f32); 2^-20 |silu(g) u| is ALLOWED for it here.  That figure
is an allowance of a few fp32 ulps (about one each for the exponential's
argument scaling, v_exp_f32 and v_rcp_f32 at the |g| < 12 of these inputs), not
a measurement; the worst |y - ref| / tol of every case is logged through the
helper's ``tag=`` (CSK_NUMERICS_LOG) so a run records how much of the bound is
used.

Grid plans.  The launcher picks the most columns per workgroup that still give
every CU a workgroup, for the plain and the gated form alike (a gated column is
two weight rows).  On 256 CUs N = 200 runs (1 column, 1 wave), 768 (1, 2),
1030 (1, 4), 3072 (2, 4), 4100 and 11008 (4, 4); 200, 1030 and 4100 end in a
ragged workgroup.  ``test_gemv_glu_grid_plans`` asserts the mapping through
``csk_gemv_plan``.

Decode attention: per-head relative error < 1.5e-2 (the figure of
tests/test_decode_gpu.py) against a float64 softmax whose query is rotated at
position kv_len - 1 and whose keys are the logical cache (what the cache holds
after the call, the appended row being the float64-rotated key rounded to
bf16); the appended key row itself within one bf16 rounding of the float64
rotation, |d| <= 2^-8 |ref| + 2^-20 (|x_j| + |x_partner|).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests._numerics import UNIT, assert_bf16_close
from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import init_random_fast_, prepare_model
from chiaswarm_amd.ops import hip_ops

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
NMAX, MMAX = 11008, 3
EPS = 1e-6


def rel_err(y, ref):
    y, ref = y.double().cpu(), ref.double().cpu()
    return ((y - ref).norm() / (ref.norm() + 1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# GEMV: RMSNorm prologue, gated form
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(K):
    """Inputs for one K, made once on the CPU and shared by every case (left
    unchanged).  ``w`` holds the gate matrix in rows [1, 1 + NMAX] and the up
    matrix in rows [NMAX + 3, ...]: two row-strided views of one tensor."""
    g = torch.Generator().manual_seed(2000 + K)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"x": (2 * r(MMAX + 1, K + 16) + 0.5).bfloat16(),
            "w": (r(2 * NMAX + 4, K + 16) / math.sqrt(K)).bfloat16(),
            "bias": (0.5 * r(NMAX)).bfloat16(),
            "res": r(MMAX, NMAX + 8).bfloat16(),
            "gamma": (1 + 0.2 * r(K)).bfloat16()}


def _views(big, M, N, K):
    return {"x": big["x"][1:1 + M, 8:8 + K], "w": big["w"][1:1 + N, 8:8 + K],
            "wu": big["w"][NMAX + 3:NMAX + 3 + N, 8:8 + K], "bias": big["bias"][:N],
            "res": big["res"][:M, 3:3 + N], "gamma": big["gamma"]}


def _case(dev, M, N, K):
    d = _data(K)
    if "dev" not in d:
        d["dev"] = {k: d[k].to(dev) for k in ("x", "w", "bias", "res", "gamma")}
    return _views(d, M, N, K), _views(d["dev"], M, N, K)


def _mm64(a, w):
    """(a @ w^T, |a| @ |w|^T) in float64, the bf16 weight rows converted a block at a time"""
    out, outs = [], []
    for i in range(0, w.shape[0], 2048):
        wb = w[i:i + 2048].double()
        out.append(a @ wb.t())
        outs.append(a.abs() @ wb.abs().t())
    return torch.cat(out, 1), torch.cat(outs, 1)


def _normed64(c, rms):
    """(x', T): the float64 RMSNorm of the rows and its absolute-value twin"""
    x = c["x"].double()
    if not rms:
        return x, x.abs()
    rstd = 1.0 / torch.sqrt((x ** 2).mean(1, keepdim=True) + EPS)
    g = c["gamma"].double()
    return x * rstd * g, x.abs() * rstd * g.abs()


def _gemv_rms_check(gpu, M, N, K, extras):
    cpu, dev = _case(gpu, M, N, K)
    buf = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=gpu)
    before = dict(hip_ops.DECODE_STATS)
    y = ops.gemv(dev["x"], dev["w"], dev["bias"] if extras else None, residual=dev["res"] if extras else None,
                 rms=(dev["gamma"], EPS), out=buf[1:1 + M, 8:8 + N])
    assert hip_ops.DECODE_STATS["gemv"] == before["gemv"] + 1, "the GEMV kernel did not run"
    assert hip_ops.DECODE_STATS["gemv_glu"] == before["gemv_glu"]
    xn, T = _normed64(cpu, True)
    ref, _ = _mm64(xn, cpu["w"])
    _, S = _mm64(T, cpu["w"])
    if extras:
        ref = ref + cpu["bias"].double() + cpu["res"].double()
        S = S + cpu["bias"].double().abs() + cpu["res"].double().abs()
    what = f"gemv rms M={M} N={N} K={K} extras={extras}"
    worst = assert_bf16_close(y, ref, S, K, what, tag=what.replace(" ", "_"))
    print(f"{what}: worst |y - ref| / tol = {worst:.3f}")
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:1 + M, 8:8 + N] = False
    assert bool((buf[keep] == SENTINEL).all()), what + ": wrote outside its output view"


@pytest.mark.parametrize("K", [8, 520, 4096])
@pytest.mark.parametrize("N", [8, 3072])
@pytest.mark.parametrize("M", [1, 3])
def test_gemv_rms_bound(gpu, M, N, K):
    for extras in (False, True):
        _gemv_rms_check(gpu, M, N, K, extras)


def test_gemv_rms_silu_and_fallbacks(gpu):
    cpu, dev = _case(gpu, 3, 200, 520)
    xn, _ = _normed64(cpu, True)
    pre = xn @ cpu["w"].double().t() + cpu["bias"].double()
    y = ops.gemv(dev["x"], dev["w"], dev["bias"], act="silu", rms=(dev["gamma"], EPS))
    assert rel_err(y, F.silu(pre)) < 5e-3
    with pytest.raises(ValueError):
        ops.gemv(dev["x"], dev["w"], ln=(dev["gamma"], None, 1e-5), rms=(dev["gamma"], EPS))
    # nine rows and the switch: a torch RMSNorm (which rounds the rows to bf16) + gemm
    d = _data(520)
    x9 = torch.cat([d["x"][:, 8:528]] * 3)[:9]
    xg = x9.to(gpu)
    rstd = 1.0 / torch.sqrt((x9.double() ** 2).mean(1, keepdim=True) + EPS)
    ref9 = (x9.double() * rstd * cpu["gamma"].double()) @ cpu["w"].double().t()
    before = dict(hip_ops.DECODE_STATS)
    assert rel_err(ops.gemv(xg, dev["w"], rms=(dev["gamma"], EPS)), ref9) < 1e-2
    hip_ops.set_decode(False)
    try:
        y1 = ops.gemv(xg[:1], dev["w"], rms=(dev["gamma"], EPS))
        y2 = ops.gemv_glu(xg[:1], dev["w"], dev["wu"], rms=(dev["gamma"], EPS))
    finally:
        hip_ops.set_decode(True)
    assert rel_err(y1, ref9[:1]) < 1e-2
    xn1 = x9[:1].double() * rstd[:1] * cpu["gamma"].double()
    assert rel_err(y2, F.silu(xn1 @ cpu["w"].double().t()) * (xn1 @ cpu["wu"].double().t())) < 1e-2
    assert hip_ops.DECODE_STATS == before, "a fallback counted as a kernel launch"


def _glu_check(gpu, M, N, K, rms):
    cpu, dev = _case(gpu, M, N, K)
    buf = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=gpu)
    before = dict(hip_ops.DECODE_STATS)
    y = ops.gemv_glu(dev["x"], dev["w"], dev["wu"], rms=(dev["gamma"], EPS) if rms else None,
                     out=buf[1:1 + M, 8:8 + N])
    assert hip_ops.DECODE_STATS["gemv_glu"] == before["gemv_glu"] + 1, "the gated GEMV kernel did not run"
    assert hip_ops.DECODE_STATS["gemv"] == before["gemv"], "a gated launch moved the plain GEMV count"
    xn, T = _normed64(cpu, rms)
    g, _ = _mm64(xn, cpu["w"])
    u, _ = _mm64(xn, cpu["wu"])
    _, Sg = _mm64(T, cpu["w"])
    _, Su = _mm64(T, cpu["wu"])
    assert float(g.abs().max()) < 12.0
    sg = F.silu(g)
    ref = sg * u
    S = 1.1 * Sg * u.abs() + sg.abs() * Su + 2.0 ** -20 * ref.abs() / ((K + 4) * UNIT)
    what = f"gemv_glu M={M} N={N} K={K} rms={rms}"
    worst = assert_bf16_close(y, ref, S, K, what, tag=what.replace(" ", "_"))
    print(f"{what}: worst |y - ref| / tol = {worst:.3f}")
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:1 + M, 8:8 + N] = False
    assert bool((buf[keep] == SENTINEL).all()), what + ": wrote outside its output view"


@pytest.mark.parametrize("K", [520, 4096])
@pytest.mark.parametrize("N", [200, 3072, 4100, 11008])
@pytest.mark.parametrize("M", [1, 3])
def test_gemv_glu_bound(gpu, M, N, K):
    for rms in (False, True):
        _glu_check(gpu, M, N, K, rms)


def _plan_by_rule(N, cus):
    for cols, nw in ((4, 4), (2, 4), (1, 4), (1, 2), (1, 1)):
        if -(-N // (cols * nw)) >= cus:
            break
    return cols, nw


def test_gemv_glu_grid_plans(gpu):
    """Every (columns, waves) plan of the launcher runs the gated kernel within
    the bound, and each N lands on the plan the module docstring names."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    on256 = {200: (1, 1), 768: (1, 2), 1030: (1, 4), 3072: (2, 4), 4100: (4, 4), 11008: (4, 4)}
    for N, plan in on256.items():
        assert hip_ops.gemv_plan(N) == _plan_by_rule(N, cus), N
        if cus == 256:
            assert hip_ops.gemv_plan(N) == plan, N
    for N in (768, 1030):  # the two plans the shapes of test_gemv_glu_bound do not reach
        _glu_check(gpu, 3, N, 520, True)
    with pytest.raises(ValueError):
        ops.gemv_glu(_case(gpu, 1, 8, 520)[1]["x"], _case(gpu, 1, 8, 520)[1]["w"], _case(gpu, 1, 16, 520)[1]["wu"])


# ---------------------------------------------------------------------------
# decode attention: RoPE, grouped heads
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rope_tables(D, P):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    f = torch.arange(P, dtype=torch.float32)[:, None] * inv[None]
    return f.cos().contiguous(), f.sin().contiguous()


def _rope64(x, cos, sin):
    """rotate-half in float64; x [..., D], cos / sin [D / 2] (the fp32 table row, exact in float64)"""
    h = x.shape[-1] // 2
    a, b = x[..., :h].double(), x[..., h:].double()
    return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)


def _attn_case(gpu, B, H, Hkv, D, S, n, append, seed, spiked, nan=True):
    """A q / k_new / v_new row (slices of one "QKV" row) and caches (slices of a
    [.., 2, Hkv, D] pair) whose rows at and past the live length hold NaN.  One
    key of the last live split is spiked by +30 in the score of the first query
    head of each group, so the combine has to rescale (``spiked=False``: plain
    random scores, where every key matters).  Cached keys are post-RoPE, so a
    cached key is spiked along the ROTATED query; the appended key is rotated at
    the query's own position, which preserves their dot product."""
    g = torch.Generator().manual_seed(seed)
    split, rep, scale = hip_ops.DECODE_SPLIT, H // Hkv, 1.0 / math.sqrt(D)
    cos, sin = _rope_tables(D, S + 8)
    c64, s64 = cos[n - 1].double(), sin[n - 1].double()
    qkv = torch.randn(B, 1, H + 2 * Hkv, D, generator=g)
    kv = torch.randn(B, S, 2, Hkv, D, generator=g)
    if spiked:
        qh = qkv[:, 0, 0:H:rep].bfloat16().float()                     # first query head of each group [B, Hkv, D]
        j = ((n - 1) // split) * split                                 # first key of the last live split
        if append and j == n - 1:
            qkv[:, 0, H:H + Hkv] += qh * (30.0 / scale) / (qh ** 2).sum(-1, keepdim=True)
        else:
            qr = _rope64(qh, c64, s64).float()
            kv[:, j, 0] += qr * (30.0 / scale) / (qr ** 2).sum(-1, keepdim=True)
    qkv, kv = qkv.bfloat16(), kv.bfloat16()
    q, kn, vn = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    full_k, full_v = kv[:, :, 0].double(), kv[:, :, 1].double()        # the logical cache after the call
    krot = None
    if append:
        krot = _rope64(kn[:, 0], c64, s64)
        full_k[:, n - 1], full_v[:, n - 1] = krot.bfloat16().double(), vn[:, 0].double()
    qr = _rope64(q, c64, s64)
    ke, ve = full_k[:, :n].repeat_interleave(rep, 2), full_v[:, :n].repeat_interleave(rep, 2)
    p = torch.softmax(torch.einsum("bqhd,bshd->bhqs", qr, ke) * scale, -1)
    ref = torch.einsum("bhqs,bshd->bqhd", p, ve)
    kv[:, (n - 1 if append else n):] = float("nan") if nan else 0.0
    return qkv.to(gpu), kv.to(gpu), (cos.to(gpu), sin.to(gpu)), ref, krot, scale


def _assert_heads_close(o, ref, what):
    assert bool(torch.isfinite(o).all()), what + ": non-finite output"
    err = (o.double().cpu() - ref).norm(dim=-1) / ref.norm(dim=-1)
    assert float(err.max()) < 1.5e-2, f"{what}: worst per-head relative error {float(err.max()):.3g} at " \
                                      f"(b, 0, h) = {tuple(int(i) for i in (err == err.max()).nonzero()[0])}"
    return float(err.max())


def _assert_appended(kc, vc, kn, vn, krot, n, what):
    """cache row n - 1: the key within one bf16 rounding of the float64 rotation, the value bit-equal"""
    got, x = kc[:, n - 1].double().cpu(), kn[:, 0].double().cpu().abs()
    h = x.shape[-1] // 2
    tol = 2.0 ** -8 * krot.abs() + 2.0 ** -20 * (x + torch.cat((x[..., h:], x[..., :h]), -1))
    bad = (got - krot).abs() > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of the appended key outside one bf16 rounding"
    assert torch.equal(_bits(vc[:, n - 1]), _bits(vn[:, 0])), what + ": appended value"


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("B", [1, 2])
def test_decode_attention_rope_gqa(gpu, B, H, Hkv, D):
    S, split = 200, hip_ops.DECODE_SPLIT
    worst = 0.0
    for n in (1, 2, split - 1, split, split + 1, S):
        for append, spiked in ((False, True), (True, True), (False, False), (True, False)):
            what = f"decode_attention rope B={B} H={H} Hkv={Hkv} D={D} kv_len={n} append={append} spiked={spiked}"
            qkv, kv, rope, ref, krot, scale = _attn_case(gpu, B, H, Hkv, D, S, n, append, n + 7 * D + H, spiked)
            q, kn, vn = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
            kc, vc = kv[:, :, 0], kv[:, :, 1]
            k0, v0 = _bits(kc).clone(), _bits(vc).clone()
            len_t = torch.tensor([n], dtype=torch.int32, device=gpu)
            kw = dict(k_new=kn, v_new=vn) if append else {}
            before = hip_ops.DECODE_STATS["decode_attention"]
            o = ops.decode_attention(q, kc, vc, scale, len_t, rope=rope, **kw)
            k1, v1 = _bits(kc).clone(), _bits(vc).clone()
            o2 = ops.decode_attention(q, kc, vc, scale, len_t, rope=rope, **kw)
            assert hip_ops.DECODE_STATS["decode_attention"] == before + 2, "the decode attention kernel did not run"
            assert o.shape == (B, 1, H, D)
            worst = max(worst, _assert_heads_close(o, ref, what))
            assert torch.equal(_bits(o), _bits(o2)), what + ": a second call differs"
            assert torch.equal(_bits(kc), k1) and torch.equal(_bits(vc), v1), what + ": a second call's caches differ"
            if append:
                _assert_appended(kc, vc, kn, vn, krot, n, what)
                k1[:, n - 1], v1[:, n - 1] = k0[:, n - 1], v0[:, n - 1]
            assert torch.equal(k1, k0) and torch.equal(v1, v0), what + ": cache rows changed"
    print(f"decode_attention rope B={B} H={H} Hkv={Hkv} D={D}: worst per-head relative error {worst:.3g}")


@pytest.mark.parametrize("D,off", [(8, False), (64, True)])
def test_decode_attention_rope_gqa_fallback(gpu, D, off):
    """D = 8 and ``set_decode(False)``: the torch steps around ``attention(kv_len=)``
    agree with the reference and count no kernel launch.  (Rows past the live
    length hold zeros: that attention kernel may load, and mask, them.)"""
    B, H, Hkv, S, n = 2, 4, 2, 200, 130
    qkv, kv, rope, ref, krot, scale = _attn_case(gpu, B, H, Hkv, D, S, n, True, 77 + D, True, nan=False)
    q, kn, vn = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    kc, vc = kv[:, :, 0], kv[:, :, 1]
    k0, v0 = _bits(kc).clone(), _bits(vc).clone()
    before = dict(hip_ops.DECODE_STATS)
    hip_ops.set_decode(not off)
    try:
        o = ops.decode_attention(q, kc, vc, scale, torch.tensor([n], dtype=torch.int32, device=gpu), k_new=kn,
                                 v_new=vn, rope=rope)
    finally:
        hip_ops.set_decode(True)
    assert hip_ops.DECODE_STATS == before
    what = f"fallback D={D} decode off={off}"
    _assert_heads_close(o, ref, what)
    _assert_appended(kc, vc, kn, vn, krot, n, what)
    k1, v1 = _bits(kc).clone(), _bits(vc).clone()
    k1[:, n - 1], v1[:, n - 1] = k0[:, n - 1], v0[:, n - 1]
    assert torch.equal(k1, k0) and torch.equal(v1, v0), what + ": cache rows changed"


# ---------------------------------------------------------------------------
# graph replay of one layer
# ---------------------------------------------------------------------------
def test_llama_layer_chain_graph_replay(gpu):
    """gemv(rms) -> decode_attention(rope, append, Hkv < H) -> gemv(residual) ->
    gemv_glu(rms) -> gemv(residual) captured once and replayed at three cache
    lengths with the input row rewritten in place: each replay equals the eager
    run bit for bit."""
    H, Hkv, D, S, FF = 4, 2, 64, 256, 688
    C, NQ = H * D, (H + 2 * Hkv) * D
    g = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    dev = lambda t: t.bfloat16().to(gpu)  # noqa: E731
    wqkv, wo = dev(r(NQ, C) / math.sqrt(C)), dev(r(C, C) / math.sqrt(C))
    wg, wu, wd = dev(r(FF, C) / math.sqrt(C)), dev(r(FF, C) / math.sqrt(C)), dev(r(C, FF) / math.sqrt(FF))
    g1, g2 = dev(1 + 0.2 * r(C)), dev(1 + 0.2 * r(C))
    kc, vc = dev(r(1, S, Hkv, D)), dev(r(1, S, Hkv, D))
    rope = tuple(t.to(gpu) for t in _rope_tables(D, S))
    x = torch.zeros(1, C, dtype=torch.bfloat16, device=gpu)
    len_t = torch.ones(1, dtype=torch.int32, device=gpu)
    scale = 1.0 / math.sqrt(D)

    def chain(x, kc, vc, len_t):
        qkv = ops.gemv(x, wqkv, rms=(g1, EPS)).view(1, 1, H + 2 * Hkv, D)
        o = ops.decode_attention(qkv[:, :, :H], kc, vc, scale, len_t, k_new=qkv[:, :, H:H + Hkv],
                                 v_new=qkv[:, :, H + Hkv:], rope=rope)
        y = ops.gemv(o.reshape(1, C), wo, residual=x)
        h = ops.gemv_glu(y, wg, wu, rms=(g2, EPS))
        return qkv, o, y, h, ops.gemv(h, wd, residual=y)

    x.copy_((2 * r(1, C) + 0.5).bfloat16())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(x, kc.clone(), vc.clone(), len_t)  # workspace allocation and lazy init outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain(x, kc, vc, len_t)
    before = dict(hip_ops.DECODE_STATS)
    for n in (1, hip_ops.DECODE_SPLIT + 1, S):
        x.copy_((2 * r(1, C) + 0.5).bfloat16())
        len_t.fill_(n)
        kc_e, vc_e = kc.clone(), vc.clone()
        graph.replay()
        eager = chain(x, kc_e, vc_e, len_t)
        for a, b, name in zip(outs, eager, ("qkv", "o", "y", "h", "out")):
            assert bool(torch.isfinite(a).all()), name
            assert torch.equal(_bits(a), _bits(b)), f"kv_len={n}: replayed {name} differs from the eager run"
        assert torch.equal(_bits(kc), _bits(kc_e)) and torch.equal(_bits(vc), _bits(vc_e))
        assert torch.equal(_bits(vc[:, n - 1]), _bits(outs[0][:, 0, H + Hkv:]))
    d = {k: hip_ops.DECODE_STATS[k] - before[k] for k in before}
    assert d == {"gemv": 9, "gemv_glu": 3, "decode_attention": 3}, d  # the eager runs; a replay calls no launcher


# ---------------------------------------------------------------------------
# LlamaLM
# ---------------------------------------------------------------------------
@torch.no_grad()
def test_llama_decode_step(gpu):
    """Prefill 20 embeddings, then 10 steps, with the kernels on and off, each
    against ``last_logits`` on the grown sequence (rel_err < 3e-2, the figure of
    test_bark_decode_step).  One eager step launches 4 L + 1 GEMV kernels, L of
    them gated (counted under their own key: 3 L + 1 plain), and L attentions."""
    from chiaswarm_amd.models.llama import LlamaConfig, LlamaLM

    c = LlamaConfig(vocab=1000, dim=256, layers=2, heads=4, kv_heads=2, ffn=688)
    with torch.device(gpu):
        m = LlamaLM(c).to(torch.bfloat16).eval().requires_grad_(False)
    init_random_fast_(m, seed=5)
    prepare_model(m)
    for lyr in m.model.layers:
        a = lyr.self_attn
        ptr = a.w_qkv.untyped_storage().data_ptr()
        assert all(p.weight.untyped_storage().data_ptr() == ptr for p in (a.q_proj, a.k_proj, a.v_proj))
        assert a.w_qkv.shape == ((c.heads + 2 * c.kv_heads) * 64, c.dim)
    gen = torch.Generator().manual_seed(6)
    seq = torch.randn(1, 20, c.dim, generator=gen).bfloat16().to(gpu)
    toks = torch.randint(0, c.vocab, (10,), generator=gen).tolist()
    full = torch.cat([seq, m.model.embed_tokens(torch.tensor([toks], device=gpu))], 1)
    refs = [m.last_logits(full[:, :21 + i]).clone() for i in range(10)]
    L = c.layers
    steps = {}
    for on in (True, False):
        hip_ops.set_decode(on)
        try:
            m._graph = None  # a captured step keeps the kernels it was captured with
            m.new_cache(30)
            assert rel_err(m.prefill(seq), m.last_logits(seq)) < 3e-2
            if on:  # one eager step: the launches of a step, counted
                before = dict(hip_ops.DECODE_STATS)
                m._decode_fn(torch.tensor([[toks[0]]], device=gpu), torch.tensor([20], device=gpu),
                             torch.tensor([21], dtype=torch.int32, device=gpu))
                d = {k: hip_ops.DECODE_STATS[k] - before[k] for k in before}
                assert d == {"gemv": 3 * L + 1, "gemv_glu": L, "decode_attention": L}, d
                assert d["gemv"] + d["gemv_glu"] == 4 * L + 1
            steps[on] = [m.decode_step(toks[i], 20 + i).clone() for i in range(10)]
        finally:
            hip_ops.set_decode(True)
            m._graph = None
    for i in range(10):
        assert steps[True][i].shape == (c.vocab,)
        assert rel_err(steps[True][i], refs[i]) < 3e-2, i
        assert rel_err(steps[False][i], refs[i]) < 3e-2, i
        assert rel_err(steps[True][i], steps[False][i]) < 3e-2, i


@torch.no_grad()
def test_instructblip_vicuna_generate_uses_decode_kernels(gpu):
    import numpy as np
    from PIL import Image

    from chiaswarm_amd.models.blip2 import Blip2Captioner, Blip2Config

    cfg = Blip2Config.from_hf({
        "model_type": "instructblip",
        "vision_config": dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                              image_size=28, patch_size=14),
        "qformer_config": dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                               encoder_hidden_size=32, cross_attention_frequency=2, vocab_size=60,
                               max_position_embeddings=32),
        "text_config": dict(model_type="llama", vocab_size=100, hidden_size=32, intermediate_size=64,
                            num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, bos_token_id=1,
                            eos_token_id=2, pad_token_id=0),
        "num_query_tokens": 4})
    m = Blip2Captioner(cfg).eval().requires_grad_(False)
    init_random_fast_(m, seed=0)
    m = m.to(gpu).to(torch.bfloat16)
    prepare_model(m)
    img = Image.fromarray((np.random.default_rng(0).random((40, 48, 3)) * 255).astype(np.uint8))
    before = dict(hip_ops.DECODE_STATS)
    out = m.generate(img, [17, 42, 5], max_length=8, qtext_ids=[3, 11, 25, 4])
    assert 2 <= len(out) <= 8, "generation ended before a decode step ran"
    # (this geometry's head dim is 8: its decode attention takes the torch fallback, the GEMVs run the kernels)
    assert all(hip_ops.DECODE_STATS[k] > before[k] for k in ("gemv", "gemv_glu")), (before, hip_ops.DECODE_STATS)
