"""The decode kernels on the GPU: the skinny-M GEMV (csrc/kernels/gemv.hip)
against a float64 reference under the per-element bf16 bound of
``tests/_numerics.py``, the split-KV decode attention (attn_decode.hip) per
head against a float64 softmax, both inside a replayed hipGraph, and Bark's
decode step wired to them.

GEMV bound.  ``assert_bf16_close(y, ref, S, K)`` requires
|y - ref| <= 2^-8 |ref| + (K + 4) 2^-22 S of every element, with ``ref`` in
float64 from the bf16 tensors and S the same expression on absolute values:

* no LayerNorm: S = |x| |W|^T + |bias| + |residual|;
* LayerNorm prologue: S = T |W|^T + |bias| + |residual| with
  T = (|x| + |mean| + mean|x|) rstd |gamma| + |beta|.  The fp32 mean, the
  centred variance and rstd each carry at most about K 2^-24 relative error, so
  a normalised element is off by at most (K + 4) 2^-24 T and the fp32 dot
  product adds the same again: half of what the helper's 2^-22 unit allows;
* act = "gelu": the fp32 term of the pre-activation value times 1.13
  (sup |gelu'| = 1.129) plus 6.5e-7, the absolute error common.h states for
  gelu_f over [-12, 12]; the inputs keep |pre-activation| < 12 (asserted).

The bound excludes no element.  Shapes are the smallest at which the kernel can
go wrong: K = 8 is one vector (63 lanes idle), 512 exactly one pass of a wave,
520 one pass plus a one-vector tail, 4096 eight passes (more than one load
batch for every column count); M = 1 / 3 / 8 the padded row counts 1 / 4 / 8.
N = 8 / 200 are single-wave workgroups of one column, 3072 two columns per wave
in four-wave workgroups; ``test_gemv_grid_plans`` adds N = 768, 1030 and 4100
for the two- and four-wave one-column plans and the four-column plan, each with
a ragged last workgroup (gemv.hip csk_gemv: the most columns per workgroup that
still give every CU a workgroup).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests._numerics import UNIT, assert_bf16_close
from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import init_random_fast_, prepare_model
from chiaswarm_amd.ops import _lib, hip_ops

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
NMAX, MMAX = 4100, 9


def rel_err(y, ref):
    y, ref = y.double().cpu(), ref.double().cpu()
    return ((y - ref).norm() / (ref.norm() + 1e-300)).item()


# ---------------------------------------------------------------------------
# GEMV
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemv_data(K):
    """Inputs for one K, made once on the CPU and shared by every case (left
    unchanged): x ~ 2 N(0,1) + 0.5 (a non-zero mean exercises the centring),
    W ~ N(0,1) / sqrt(K), all as bf16, wider / taller than any case so that the
    cases take strided slices."""
    g = torch.Generator().manual_seed(1000 + K)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = {"x": (2 * r(MMAX + 1, K + 16) + 0.5).bfloat16(),
         "w": (r(NMAX + 2, K + 16) / math.sqrt(K)).bfloat16(),
         "bias": (0.5 * r(NMAX)).bfloat16(),
         "res": r(MMAX, NMAX + 8).bfloat16(),
         "gamma": (1 + 0.2 * r(K)).bfloat16(),
         "beta": (0.2 * r(K)).bfloat16()}
    d["w64"] = d["w"].double()
    return d


def _gemv_case(dev, M, N, K):
    d = _gemv_data(K)
    cpu = {"x": d["x"][1:1 + M, 8:8 + K], "w": d["w"][1:1 + N, 8:8 + K], "bias": d["bias"][:N],
           "res": d["res"][:M, 3:3 + N], "gamma": d["gamma"], "beta": d["beta"]}
    if "dev" not in d:
        d["dev"] = {k: d[k].to(dev) for k in ("x", "w", "bias", "res", "gamma", "beta")}
    big = d["dev"]
    gpu = {"x": big["x"][1:1 + M, 8:8 + K], "w": big["w"][1:1 + N, 8:8 + K], "bias": big["bias"][:N],
           "res": big["res"][:M, 3:3 + N], "gamma": big["gamma"], "beta": big["beta"]}
    cpu["w64"] = d["w64"][1:1 + N, 8:8 + K]
    return cpu, gpu


def _gemv_check(gpu, M, N, K, extras, act, ln):
    cpu, dev = _gemv_case(gpu, M, N, K)
    buf = torch.full((M + 2, N + 16), SENTINEL, dtype=torch.bfloat16, device=gpu)
    out = buf[1:1 + M, 8:8 + N]
    before = hip_ops.DECODE_STATS["gemv"]
    y = ops.gemv(dev["x"], dev["w"], dev["bias"] if extras else None, act=act,
                 residual=dev["res"] if extras else None,
                 ln=(dev["gamma"], dev["beta"], 1e-5) if ln else None, out=out)
    assert hip_ops.DECODE_STATS["gemv"] == before + 1, "the GEMV kernel did not run"
    ref, S = _gemv_ref(cpu, extras, extras, act, ln)
    what = f"gemv M={M} N={N} K={K} extras={extras} act={act} ln={ln}"
    worst = assert_bf16_close(y, ref, S, K, what, tag=what.replace(" ", "_"))
    print(f"{what}: worst |y - ref| / tol = {worst:.3f}")
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:1 + M, 8:8 + N] = False
    assert bool((buf[keep] == SENTINEL).all()), what + ": wrote outside its output view"


def _gemv_ref(c, bias, res, act, ln, eps=1e-5):
    """(ref, S) in float64 on the CPU; S folds the activation's terms so that the
    helper's (K + 4) 2^-22 S is the bound of the module docstring."""
    x, w = c["x"].double(), c["w64"]
    K = x.shape[1]
    if ln:
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        g, b = c["gamma"].double(), c["beta"].double()
        xn = (x - mean) * rstd * g + b
        T = (x.abs() + mean.abs() + x.abs().mean(1, keepdim=True)) * rstd * g.abs() + b.abs()
    else:
        xn, T = x, x.abs()
    pre = xn @ w.t()
    S = T @ w.abs().t()
    if bias:
        pre = pre + c["bias"].double()
        S = S + c["bias"].double().abs()
    if act == "gelu":
        assert float(pre.abs().max()) < 12.0
        ref = F.gelu(pre)
        S = 1.13 * S + 6.5e-7 / ((K + 4) * UNIT)
    else:
        ref = pre
    if res:
        ref = ref + c["res"].double()
        S = S + c["res"].double().abs()
    return ref, S


@pytest.mark.parametrize("K", [8, 512, 520, 4096])
@pytest.mark.parametrize("N", [8, 200, 3072])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_gemv_bound(gpu, M, N, K):
    for extras in (False, True):
        for act in (None, "gelu"):
            for ln in (False, True):
                _gemv_check(gpu, M, N, K, extras, act, ln)


@pytest.mark.parametrize("N", [768, 1030, 4100])
def test_gemv_grid_plans(gpu, N):
    for M, extras, act, ln in ((1, False, None, True), (3, True, "gelu", True), (8, True, None, False)):
        _gemv_check(gpu, M, N, 520, extras, act, ln)


def test_gemv_ln_without_beta_and_other_acts(gpu):
    cpu, dev = _gemv_case(gpu, 3, 200, 520)
    y = ops.gemv(dev["x"], dev["w"], ln=(dev["gamma"], None, 1e-5))
    c2 = dict(cpu, beta=torch.zeros_like(cpu["beta"]))
    ref, S = _gemv_ref(c2, False, False, None, True)
    assert_bf16_close(y, ref, S, 520, "gemv ln without beta")
    pre, _ = _gemv_ref(cpu, True, False, None, False)
    for act in ("silu", "quick_gelu", "relu"):
        y = ops.gemv(dev["x"], dev["w"], dev["bias"], act=act)
        assert rel_err(y, ops.apply_act(pre, act)) < 5e-3, act


def test_gemv_nine_rows_take_the_fallback(gpu):
    d = _gemv_data(520)
    N, K = 200, 520
    x, w = d["x"][:9, 8:8 + K], d["w"][1:1 + N, 8:8 + K]
    c = {"x": x, "w64": d["w64"][1:1 + N, 8:8 + K], "bias": d["bias"][:N], "res": d["res"][:9, 3:3 + N],
         "gamma": d["gamma"], "beta": d["beta"]}
    _gemv_case(gpu, 1, 8, 520)
    t = d["dev"]
    xg, wg = t["x"][:9, 8:8 + K], t["w"][1:1 + N, 8:8 + K]
    before = hip_ops.DECODE_STATS["gemv"]
    y = ops.gemv(xg, wg, t["bias"][:N], residual=t["res"][:9, 3:3 + N])
    ref, S = _gemv_ref(c, True, True, None, False)
    assert_bf16_close(y, ref, S, K, "gemv M=9 (gemm fallback)")
    # with a LayerNorm the fallback is the layer_norm kernel (which rounds to bf16) + gemm
    y = ops.gemv(xg, wg, t["bias"][:N], act="gelu", ln=(t["gamma"], t["beta"], 1e-5))
    ref, _ = _gemv_ref(c, True, False, "gelu", True)
    assert rel_err(y, ref) < 1e-2
    assert hip_ops.DECODE_STATS["gemv"] == before
    # an odd K and the switch take it too
    y = ops.gemv(t["x"][:2, :10], t["w"][:16, :10])
    assert rel_err(y, d["x"][:2, :10].double() @ d["w64"][:16, :10].t()) < 1e-2
    hip_ops.set_decode(False)
    try:
        y = ops.gemv(xg[:1], wg)
    finally:
        hip_ops.set_decode(True)
    assert rel_err(y, x[:1].double() @ c["w64"].t()) < 1e-2
    assert hip_ops.DECODE_STATS["gemv"] == before


# ---------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------
def _attn_ref(q, k, v, scale, n):
    """float64 softmax over the first n keys; [B, 1, H, D] on the CPU"""
    q, k, v = q.double().cpu(), k[:, :n].double().cpu(), v[:, :n].double().cpu()
    s = torch.einsum("bqhd,bshd->bhqs", q, k) * scale
    return torch.einsum("bhqs,bshd->bqhd", torch.softmax(s, -1), v)


def _assert_heads_close(o, ref, what):
    assert bool(torch.isfinite(o).all()), what + ": non-finite output"
    err = (o.double().cpu() - ref).norm(dim=-1) / ref.norm(dim=-1)
    assert float(err.max()) < 1.5e-2, f"{what}: worst per-head relative error {float(err.max()):.3g} at " \
                                      f"(b, 0, h) = {tuple(int(i) for i in (err == err.max()).nonzero()[0])}"
    return float(err.max())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _attn_case(gpu, B, H, D, S, n, append, seed, spiked=True):
    """Caches whose rows at and past n hold NaN (with an append: at and past
    n - 1, the appended row arrives in k_new / v_new), one key of the last live
    split spiked by +30 in score, so the combine has to rescale the others
    (``spiked=False``: plain random scores, where every key matters)."""
    g = torch.Generator().manual_seed(seed)
    split = hip_ops.DECODE_SPLIT
    scale = 1.0 / math.sqrt(D)
    # views of wider tensors: q / k_new / v_new are slices of one "QKV" row, the caches of a [.., 2, H, D] pair
    qkv = torch.randn(B, 1, 3, H, D, generator=g)
    kv = torch.randn(B, S, 2, H, D, generator=g)
    j = ((n - 1) // split) * split  # first key of the last live split
    spike = qkv[:, 0, 0] * (30.0 / scale) / (qkv[:, 0, 0] ** 2).sum(-1, keepdim=True)
    if not spiked:  # every live key carries weight: a dropped key, split or head shows
        pass
    elif append and j == n - 1:
        qkv[:, 0, 1] += spike
    else:
        kv[:, j, 0] += spike
    qkv, kv = qkv.bfloat16().to(gpu), kv.bfloat16().to(gpu)
    full_k, full_v = kv[:, :, 0].clone(), kv[:, :, 1].clone()  # what the cache holds logically after the call
    if append:
        full_k[:, n - 1], full_v[:, n - 1] = qkv[:, 0, 1], qkv[:, 0, 2]
    live = n - 1 if append else n
    kv[:, live:] = float("nan")
    return qkv, kv, full_k, full_v, scale


@pytest.mark.parametrize("S", [64, 1024, 1200])
@pytest.mark.parametrize("H,D", [(2, 32), (16, 64), (4, 128)])
@pytest.mark.parametrize("B", [1, 2])
def test_decode_attention(gpu, B, H, D, S):
    split = hip_ops.DECODE_SPLIT
    assert _lib.call_int("csk_attn_decode_split") == split
    worst = 0.0
    for n in sorted({1, 2, split - 1, split, split + 1, S} & set(range(1, S + 1))):
        for append, spiked in ((False, True), (True, True), (False, False), (True, False)):
            what = f"decode_attention B={B} H={H} D={D} S={S} kv_len={n} append={append} spiked={spiked}"
            qkv, kv, full_k, full_v, scale = _attn_case(gpu, B, H, D, S, n, append, n + 7 * S + D, spiked)
            q, kn, vn = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
            kc, vc = kv[:, :, 0], kv[:, :, 1]
            k0, v0 = _bits(kc).clone(), _bits(vc).clone()
            len_t = torch.tensor([n], dtype=torch.int32, device=gpu)
            kw = dict(k_new=kn, v_new=vn) if append else {}
            before = hip_ops.DECODE_STATS["decode_attention"]
            o = ops.decode_attention(q, kc, vc, scale, len_t, **kw)
            o2 = ops.decode_attention(q, kc, vc, scale, len_t, **kw)
            assert hip_ops.DECODE_STATS["decode_attention"] == before + 2, "the decode attention kernel did not run"
            assert o.shape == (B, 1, H, D)
            worst = max(worst, _assert_heads_close(o, _attn_ref(q, full_k, full_v, scale, n), what))
            assert torch.equal(_bits(o), _bits(o2)), what + ": a second call differs (arrival counter not reset?)"
            k1, v1 = _bits(kc), _bits(vc)
            if append:
                assert torch.equal(k1[:, n - 1], _bits(kn[:, 0])) and torch.equal(v1[:, n - 1], _bits(vn[:, 0])), \
                    what + ": appended row"
                k1, v1 = k1.clone(), v1.clone()
                k1[:, n - 1], v1[:, n - 1] = k0[:, n - 1], v0[:, n - 1]
            assert torch.equal(k1, k0) and torch.equal(v1, v0), what + ": cache rows changed"
    print(f"decode_attention B={B} H={H} D={D} S={S}: worst per-head relative error {worst:.3g}")


def test_decode_attention_empty_and_errors(gpu):
    qkv, kv, _, _, scale = _attn_case(gpu, 2, 16, 64, 1024, 1, False, seed=5)
    q, kc, vc = qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1]
    k0 = _bits(kc).clone()
    for n in (0, -3):
        o = ops.decode_attention(q, kc, vc, scale, torch.tensor([n], dtype=torch.int32, device=gpu),
                                 k_new=qkv[:, :, 1], v_new=qkv[:, :, 2])
        assert o.shape == q.shape and not bool(o.any())
    assert torch.equal(_bits(kc), k0)
    # a length past the capacity is clamped to it
    kv2 = torch.randn(2, 64, 2, 16, 64, device=gpu).bfloat16()
    o = ops.decode_attention(q, kv2[:, :, 0], kv2[:, :, 1], scale, torch.tensor([900], dtype=torch.int32, device=gpu))
    _assert_heads_close(o, _attn_ref(q, kv2[:, :, 0], kv2[:, :, 1], scale, 64), "kv_len past S")
    with pytest.raises(TypeError):
        ops.decode_attention(q, kc, vc, scale, torch.tensor([3], device=gpu))
    with pytest.raises(TypeError):
        ops.decode_attention(q, kc, vc, scale, torch.tensor([3], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, scale, torch.tensor([3], dtype=torch.int32, device=gpu),
                             k_new=qkv[:, :, 1, :8], v_new=qkv[:, :, 2])


def test_decode_attention_switch_off_matches(gpu):
    n = 130
    qkv, kv, full_k, full_v, scale = _attn_case(gpu, 1, 16, 64, 1024, n, True, seed=11)
    kv[:, n - 1:] = 0  # the fallback's attention kernel may load (and mask) rows past kv_len
    len_t = torch.tensor([n], dtype=torch.int32, device=gpu)
    before = hip_ops.DECODE_STATS["decode_attention"]
    hip_ops.set_decode(False)
    try:
        o = ops.decode_attention(qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1], scale, len_t, k_new=qkv[:, :, 1],
                                 v_new=qkv[:, :, 2])
    finally:
        hip_ops.set_decode(True)
    assert hip_ops.DECODE_STATS["decode_attention"] == before
    _assert_heads_close(o, _attn_ref(qkv[:, :, 0], full_k, full_v, scale, n), "decode off")
    assert torch.equal(_bits(kv[:, n - 1, 0]), _bits(qkv[:, 0, 1]))


# ---------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------
def test_decode_chain_graph_replay(gpu):
    """gemv(ln) -> decode_attention(append) -> gemv(residual) captured once and
    replayed at three cache lengths with the input row rewritten in place: each
    replay equals the eager run bit for bit and the float64 reference stage by
    stage."""
    H, D, S = 4, 64, 256
    C = H * D
    g = torch.Generator().manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    wqkv, wo = (r(3 * C, C) / math.sqrt(C)).bfloat16().to(gpu), (r(C, C) / math.sqrt(C)).bfloat16().to(gpu)
    gamma, beta = (1 + 0.2 * r(C)).bfloat16().to(gpu), (0.2 * r(C)).bfloat16().to(gpu)
    kc, vc = r(1, S, H, D).bfloat16().to(gpu), r(1, S, H, D).bfloat16().to(gpu)
    x = torch.zeros(1, C, dtype=torch.bfloat16, device=gpu)
    len_t = torch.ones(1, dtype=torch.int32, device=gpu)
    scale = 1.0 / math.sqrt(D)

    def chain(x, kc, vc, len_t):
        qkv = ops.gemv(x, wqkv, ln=(gamma, beta, 1e-5))
        v5 = qkv.view(1, 1, 3, H, D)
        o = ops.decode_attention(v5[:, :, 0], kc, vc, scale, len_t, k_new=v5[:, :, 1], v_new=v5[:, :, 2])
        return qkv, o, ops.gemv(o.reshape(1, C), wo, residual=x)

    x.copy_((2 * r(1, C) + 0.5).bfloat16())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(x, kc.clone(), vc.clone(), len_t)  # workspace allocation and lazy init outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain(x, kc, vc, len_t)
    for n in (1, hip_ops.DECODE_SPLIT + 1, S):
        x.copy_((2 * r(1, C) + 0.5).bfloat16())
        len_t.fill_(n)
        kc_e, vc_e = kc.clone(), vc.clone()
        graph.replay()
        eager = chain(x, kc_e, vc_e, len_t)
        for a, b, name in zip(outs, eager, ("qkv", "o", "y")):
            assert torch.equal(_bits(a), _bits(b)), f"kv_len={n}: replayed {name} differs from the eager run"
        assert torch.equal(_bits(kc), _bits(kc_e)) and torch.equal(_bits(vc), _bits(vc_e))
        qkv, o, y = outs
        c = {"x": x.cpu(), "w64": wqkv.double().cpu(), "gamma": gamma.cpu(), "beta": beta.cpu()}
        ref, S_ = _gemv_ref(c, False, False, None, True)
        assert_bf16_close(qkv, ref, S_, C, f"graph qkv kv_len={n}")
        v5 = qkv.view(1, 1, 3, H, D)
        assert torch.equal(_bits(kc[:, n - 1]), _bits(v5[:, 0, 1]))
        _assert_heads_close(o, _attn_ref(v5[:, :, 0], kc, vc, scale, n), f"graph o kv_len={n}")
        c = {"x": o.reshape(1, C).cpu(), "w64": wo.double().cpu(), "res": x.cpu()}
        ref, S_ = _gemv_ref(c, False, True, None, False)
        assert_bf16_close(y, ref, S_, C, f"graph y kv_len={n}")


# ---------------------------------------------------------------------------
# Bark
# ---------------------------------------------------------------------------
@torch.no_grad()
def test_bark_decode_step(gpu):
    from chiaswarm_amd.models import bark as bk

    sc, _, _ = bk.bark_configs("small")
    with torch.device(gpu):
        m = bk.BarkCausalGPT(sc).to(torch.bfloat16).eval().requires_grad_(False)
    init_random_fast_(m, seed=3)
    prepare_model(m)
    ids = torch.randint(0, 10000, (1, 40), device=gpu)
    m.cache = None
    full = m(ids, last_only=False)
    steps = {}
    for on in (True, False):
        hip_ops.set_decode(on)
        try:
            m._graph = None  # a captured step keeps the kernels it was captured with
            m.new_cache()
            m(ids[:, :30], pos=0)
            if on:  # one eager step: the launches of a step, counted
                L = sc.n_layer
                g0, a0 = hip_ops.DECODE_STATS["gemv"], hip_ops.DECODE_STATS["decode_attention"]
                m._decode_fn(ids[:, 30:31], torch.tensor([30], device=gpu),
                             torch.tensor([31], dtype=torch.int32, device=gpu))
                assert hip_ops.DECODE_STATS["gemv"] - g0 == 4 * L + 1
                assert hip_ops.DECODE_STATS["decode_attention"] - a0 == L
            steps[on] = [m.decode_step(int(ids[0, i]), i)[0].clone() for i in range(30, 40)]
        finally:
            hip_ops.set_decode(True)
            m._graph = None
    for j, i in enumerate(range(30, 40)):
        assert rel_err(steps[True][j], full[0, i]) < 3e-2, i
        assert rel_err(steps[False][j], full[0, i]) < 3e-2, i
        assert rel_err(steps[True][j], steps[False][j]) < 3e-2, i


@torch.no_grad()
def test_bark_tiny_generate_uses_decode_kernels(gpu):
    from chiaswarm_amd.models.bark import Bark

    g0, a0 = hip_ops.DECODE_STATS["gemv"], hip_ops.DECODE_STATS["decode_attention"]
    b = Bark(str(gpu), size="tiny")
    a = b.generate_audio("hello", seed=0, max_semantic_tokens=16)
    assert a.ndim == 1 and len(a) > 0
    assert hip_ops.DECODE_STATS["gemv"] > g0 and hip_ops.DECODE_STATS["decode_attention"] > a0
