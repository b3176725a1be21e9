"""The decode attention's head dim 80 and distance-indexed score bias
(``rel_bias=``, csrc/kernels/attn_decode.hip) on the GPU, the T5- and
OPT-shaped layer chains inside a replayed hipGraph, and the KV-cached decode of
``T5Seq2Seq`` and of BLIP-2's OPT language model wired to them.  Conventions of
tests/test_llama_decode_gpu.py: q / k_new / v_new are slices of one QKV row,
the caches slices of a [.., 2, Hkv, D] pair with NaN at and past the live
length, ``DECODE_STATS`` proves that the kernel ran, references are float64
softmaxes of the bf16 tensors.

Decode attention: per-head relative error < 1.5e-2 (the figure of
tests/test_decode_gpu.py) against

    softmax_j(q . k_j * scale + rel_bias[h, n - 1 - j]) v_j,   j < n,

the keys being the logical cache (what the cache holds after the call).  The
table is a contiguous fp32 [H, S + 8] tensor of uniform entries in [-8, 8];
entries at distances >= n, which the query cannot reach, hold NaN.  Without
RoPE the appended key row must be bit-equal to ``k_new``.

Spikes.  "key": the first key of the last live split is moved by +30 in the
score of the first query head of each group (tests/test_llama_decode_gpu.py).
"bias": the table entry of that key's distance is raised by 30 for every head,
the keys staying plain, so the split combine has to rescale because of the bias
alone.

Model steps: rel_err < 3e-2 against the re-run logits on the grown sequence,
the figure of ``test_llama_decode_step``.  The T5 geometry's q projections are
scaled by d_kv^-0.5 after the random init: T5 has no 1 / sqrt(d_kv) in its
scores and folds that factor into the initialisation of q (transformers'
``T5PreTrainedModel._init_weights``: std (d_model d_kv)^-0.5 for q against
d_model^-0.5 for k), so unit-variance scores are what the architecture runs at.
"""
import dataclasses
import functools
import math

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import init_random_fast_, prepare_model
from chiaswarm_amd.ops import hip_ops

pytestmark = pytest.mark.gpu

EPS = 1e-6


def rel_err(y, ref):
    y, ref = y.double().cpu(), ref.double().cpu()
    return ((y - ref).norm() / (ref.norm() + 1e-300)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _stats_delta(before):
    return {k: hip_ops.DECODE_STATS[k] - before[k] for k in before}


@functools.lru_cache(maxsize=None)
def _rope_tables(D, P):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    f = torch.arange(P, dtype=torch.float32)[:, None] * inv[None]
    return f.cos().contiguous(), f.sin().contiguous()


def _rope64(x, cos, sin):
    h = x.shape[-1] // 2
    a, b = x[..., :h].double(), x[..., h:].double()
    return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)


def _attn_case(gpu, B, H, Hkv, D, S, n, append, seed, spike, bias=True, nan=True, rope=False):
    """One decode-attention case and its float64 reference (module docstring).
    ``spike``: None, "key" or "bias"; ``rope``: the query and the appended key
    are rotated at position n - 1 (fallback cases only; spike is then not
    "key", so no cached key has to be built along a rotated query)."""
    g = torch.Generator().manual_seed(seed)
    split, rep, scale = hip_ops.DECODE_SPLIT, H // Hkv, 1.0 / math.sqrt(D)
    qkv = torch.randn(B, 1, H + 2 * Hkv, D, generator=g)
    kv = torch.randn(B, S, 2, Hkv, D, generator=g)
    rb = 8 * (2 * torch.rand(H, S + 8, generator=g) - 1)
    j = ((n - 1) // split) * split                                     # first key of the last live split
    if spike == "key":
        assert not rope
        qh = qkv[:, 0, 0:H:rep].bfloat16().float()                     # first query head of each group [B, Hkv, D]
        d = qh * (30.0 / scale) / (qh ** 2).sum(-1, keepdim=True)
        if append and j == n - 1:
            qkv[:, 0, H:H + Hkv] += d
        else:
            kv[:, j, 0] += d
    elif spike == "bias":
        rb[:, n - 1 - j] += 30.0
    qkv, kv = qkv.bfloat16(), kv.bfloat16()
    q, kn, vn = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    cos, sin = _rope_tables(D, S + 8)
    c64, s64 = cos[n - 1].double(), sin[n - 1].double()
    full_k, full_v = kv[:, :, 0].double(), kv[:, :, 1].double()        # the logical cache after the call
    if append:
        full_k[:, n - 1] = _rope64(kn[:, 0], c64, s64).bfloat16().double() if rope else kn[:, 0].double()
        full_v[:, n - 1] = vn[:, 0].double()
    q64 = _rope64(q, c64, s64) if rope else q.double()
    ke, ve = full_k[:, :n].repeat_interleave(rep, 2), full_v[:, :n].repeat_interleave(rep, 2)
    s = torch.einsum("bqhd,bshd->bhqs", q64, ke) * scale
    if bias:
        s = s + rb[:, torch.arange(n - 1, -1, -1)].double()[None, :, None]
    ref = torch.einsum("bhqs,bshd->bqhd", torch.softmax(s, -1), ve)
    kv[:, (n - 1 if append else n):] = float("nan") if nan else 0.0
    rb[:, n:] = float("nan")
    return dict(qkv=qkv.to(gpu), kv=kv.to(gpu), rb=rb.contiguous().to(gpu) if bias else None, ref=ref, scale=scale,
                rope=(cos.to(gpu), sin.to(gpu)) if rope else None)


def _assert_heads_close(o, ref, what):
    assert bool(torch.isfinite(o).all()), what + ": non-finite output"
    err = (o.double().cpu() - ref).norm(dim=-1) / ref.norm(dim=-1)
    worst = float(err.max())
    print(f"{what}: worst per-head relative error {worst:.3g}")
    assert worst < 1.5e-2, f"{what}: worst per-head relative error {worst:.3g} at (b, 0, h) = " \
                           f"{tuple(int(i) for i in (err == err.max()).nonzero()[0])}"
    return worst


@pytest.mark.parametrize("D,bias", [(32, True), (64, True), (80, True), (128, True), (80, False)])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("B", [1, 2])
def test_decode_attention_rel_bias_and_d80(gpu, B, H, Hkv, D, bias):
    S, split = 200, hip_ops.DECODE_SPLIT
    for n in (1, 2, split - 1, split, split + 1, S):
        for append in (False, True):
            for spike in ("key", "bias", None) if bias else ("key", None):
                what = f"decode_attention B={B} H={H} Hkv={Hkv} D={D} bias={bias} kv_len={n} append={append} " \
                       f"spike={spike}"
                c = _attn_case(gpu, B, H, Hkv, D, S, n, append, n + 7 * D + H + (3 if bias else 0), spike, bias)
                qkv, kv = c["qkv"], c["kv"]
                q, kn, vn = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
                kc, vc = kv[:, :, 0], kv[:, :, 1]
                k0, v0 = _bits(kc).clone(), _bits(vc).clone()
                len_t = torch.tensor([n], dtype=torch.int32, device=gpu)
                kw = dict(k_new=kn, v_new=vn) if append else {}
                before = hip_ops.DECODE_STATS["decode_attention"]
                o = ops.decode_attention(q, kc, vc, c["scale"], len_t, rel_bias=c["rb"], **kw)
                assert hip_ops.DECODE_STATS["decode_attention"] == before + 1, "the decode attention kernel did not run"
                k1, v1 = _bits(kc).clone(), _bits(vc).clone()
                o2 = ops.decode_attention(q, kc, vc, c["scale"], len_t, rel_bias=c["rb"], **kw)
                assert hip_ops.DECODE_STATS["decode_attention"] == before + 2
                assert o.shape == (B, 1, H, D)
                _assert_heads_close(o, c["ref"], what)
                assert torch.equal(_bits(o), _bits(o2)), what + ": a second call differs"
                assert torch.equal(_bits(kc), k1) and torch.equal(_bits(vc), v1), what + ": a second call's caches"
                if append:
                    assert torch.equal(_bits(kc[:, n - 1]), _bits(kn[:, 0])), what + ": appended key"
                    assert torch.equal(_bits(vc[:, n - 1]), _bits(vn[:, 0])), what + ": appended value"
                    k1[:, n - 1], v1[:, n - 1] = k0[:, n - 1], v0[:, n - 1]
                assert torch.equal(k1, k0) and torch.equal(v1, v0), what + ": cache rows changed"


@pytest.mark.parametrize("D,off,rope", [(16, False, False), (64, True, False), (80, True, False), (80, False, True)])
def test_decode_attention_rel_bias_fallbacks(gpu, D, off, rope):
    """D = 16, ``set_decode(False)`` and D = 80 with ``rope=``: the torch steps
    around ``attention(bias=, kv_lens=)`` agree with the reference and count no
    kernel launch.  (Rows past the live length hold zeros: that attention
    kernel may load, and mask, them.)"""
    B, H, Hkv, S = 2, 4, 2, 200
    for n in (1, 130, S):
        for append in (False, True):
            what = f"fallback D={D} decode off={off} rope={rope} kv_len={n} append={append}"
            c = _attn_case(gpu, B, H, Hkv, D, S, n, append, 77 + D + n, "bias", nan=False, rope=rope)
            qkv, kv = c["qkv"], c["kv"]
            q, kn, vn = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
            kc, vc = kv[:, :, 0], kv[:, :, 1]
            k0, v0 = _bits(kc).clone(), _bits(vc).clone()
            kw = dict(k_new=kn, v_new=vn) if append else {}
            before = dict(hip_ops.DECODE_STATS)
            hip_ops.set_decode(not off)
            try:
                o = ops.decode_attention(q, kc, vc, c["scale"], torch.tensor([n], dtype=torch.int32, device=gpu),
                                         rel_bias=c["rb"], rope=c["rope"], **kw)
            finally:
                hip_ops.set_decode(True)
            assert hip_ops.DECODE_STATS == before, what + ": a fallback counted as a kernel launch"
            _assert_heads_close(o, c["ref"], what)
            k1, v1 = _bits(kc).clone(), _bits(vc).clone()
            if append:
                assert torch.equal(_bits(vc[:, n - 1]), _bits(vn[:, 0])), what + ": appended value"
                if not rope:
                    assert torch.equal(_bits(kc[:, n - 1]), _bits(kn[:, 0])), what + ": appended key"
                k1[:, n - 1], v1[:, n - 1] = k0[:, n - 1], v0[:, n - 1]
            assert torch.equal(k1, k0) and torch.equal(v1, v0), what + ": cache rows changed"


# ---------------------------------------------------------------------------
# graph replay of one layer
# ---------------------------------------------------------------------------
def _replay_check(gpu, chain, names, x, kc, vc, len_t, S, new_x, expect):
    """Capture ``chain`` once and replay it at three cache lengths with the input
    row rewritten in place: every output and both caches equal the eager run bit
    for bit; ``expect``: the launches of the three eager runs."""
    x.copy_(new_x())
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
        x.copy_(new_x())
        len_t.fill_(n)
        kc_e, vc_e = kc.clone(), vc.clone()
        graph.replay()
        eager = chain(x, kc_e, vc_e, len_t)
        for a, b, name in zip(outs, eager, names):
            assert bool(torch.isfinite(a).all()), name
            assert torch.equal(_bits(a), _bits(b)), f"kv_len={n}: replayed {name} differs from the eager run"
        assert torch.equal(_bits(kc), _bits(kc_e)) and torch.equal(_bits(vc), _bits(vc_e))
        assert torch.equal(_bits(kc[:, n - 1]), _bits(outs[0][:, 0, 1])), "appended key"
        assert torch.equal(_bits(vc[:, n - 1]), _bits(outs[0][:, 0, 2])), "appended value"
    assert _stats_delta(before) == expect, _stats_delta(before)  # the eager runs; a replay calls no launcher


def test_t5_layer_chain_graph_replay(gpu):
    """gemv(rms) -> decode_attention(rel_bias, append) -> gemv(residual) ->
    gemv(rms) -> cross decode_attention over 37 of 256 encoder rows ->
    gemv(residual) -> gemv_glu(gelu_tanh, rms) -> gemv(residual)."""
    H, D, S, ES, EN, FF = 4, 64, 256, 256, 37, 512
    C = H * D
    g = torch.Generator().manual_seed(41)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    dev = lambda t: t.bfloat16().to(gpu)  # noqa: E731
    wqkv, wo = dev(r(3 * C, C) / math.sqrt(C) / 2), dev(r(C, C) / math.sqrt(C))
    wq2, wo2 = dev(r(C, C) / math.sqrt(C) / 2), dev(r(C, C) / math.sqrt(C))
    wi0, wi1, wd = dev(r(FF, C) / math.sqrt(C)), dev(r(FF, C) / math.sqrt(C)), dev(r(C, FF) / math.sqrt(FF))
    g1, g2, g3 = dev(1 + 0.2 * r(C)), dev(1 + 0.2 * r(C)), dev(1 + 0.2 * r(C))
    kc, vc = dev(r(1, S, H, D) / 2), dev(r(1, S, H, D))
    xkv = r(1, ES, 2, H, D) / 2
    xkv[:, EN:] = float("nan")  # encoder rows past the live length are never read
    xkv = dev(xkv)
    tab = (2 * r(H, S)).to(gpu)
    enc_len = torch.tensor([EN], dtype=torch.int32, device=gpu)
    x = torch.zeros(1, C, dtype=torch.bfloat16, device=gpu)
    len_t = torch.ones(1, dtype=torch.int32, device=gpu)

    def chain(x, kc, vc, len_t):
        qkv = ops.gemv(x, wqkv, rms=(g1, EPS)).view(1, 1, 3, H, D)
        o = ops.decode_attention(qkv[:, :, 0], kc, vc, 1.0, len_t, k_new=qkv[:, :, 1], v_new=qkv[:, :, 2],
                                 rel_bias=tab)
        y = ops.gemv(o.reshape(1, C), wo, residual=x)
        q2 = ops.gemv(y, wq2, rms=(g2, EPS)).view(1, 1, H, D)
        o2 = ops.decode_attention(q2, xkv[:, :, 0], xkv[:, :, 1], 1.0, enc_len)
        y2 = ops.gemv(o2.reshape(1, C), wo2, residual=y)
        h = ops.gemv_glu(y2, wi0, wi1, act="gelu_tanh", rms=(g3, EPS))
        return qkv, o, y, q2, o2, y2, h, ops.gemv(h, wd, residual=y2)

    _replay_check(gpu, chain, ("qkv", "o", "y", "q2", "o2", "y2", "h", "out"), x, kc, vc, len_t, S,
                  lambda: (2 * r(1, C) + 0.5).bfloat16(), {"gemv": 15, "gemv_glu": 3, "decode_attention": 6})


def test_opt_layer_chain_graph_replay(gpu):
    """gemv(ln, bias) -> decode_attention(append) at D = 80 -> gemv(bias,
    residual) -> gemv(ln, bias, relu) -> gemv(bias, residual)."""
    H, D, S, FF = 4, 80, 256, 640
    C = H * D
    g = torch.Generator().manual_seed(43)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    dev = lambda t: t.bfloat16().to(gpu)  # noqa: E731
    w_in, b_in = dev(r(3 * C, C) / math.sqrt(C)), dev(0.1 * r(3 * C))
    wo, bo = dev(r(C, C) / math.sqrt(C)), dev(0.1 * r(C))
    w1, b1 = dev(r(FF, C) / math.sqrt(C)), dev(0.1 * r(FF))
    w2, b2 = dev(r(C, FF) / math.sqrt(FF)), dev(0.1 * r(C))
    ln1, ln2 = (dev(1 + 0.2 * r(C)), dev(0.1 * r(C)), 1e-5), (dev(1 + 0.2 * r(C)), dev(0.1 * r(C)), 1e-5)
    kc, vc = dev(r(1, S, H, D)), dev(r(1, S, H, D))
    x = torch.zeros(1, C, dtype=torch.bfloat16, device=gpu)
    len_t = torch.ones(1, dtype=torch.int32, device=gpu)
    scale = D ** -0.5

    def chain(x, kc, vc, len_t):
        qkv = ops.gemv(x, w_in, b_in, ln=ln1).view(1, 1, 3, H, D)
        o = ops.decode_attention(qkv[:, :, 0], kc, vc, scale, len_t, k_new=qkv[:, :, 1], v_new=qkv[:, :, 2])
        y = ops.gemv(o.reshape(1, C), wo, bo, residual=x)
        h = ops.gemv(y, w1, b1, act="relu", ln=ln2)
        return qkv, o, y, h, ops.gemv(h, w2, b2, residual=y)

    _replay_check(gpu, chain, ("qkv", "o", "y", "h", "out"), x, kc, vc, len_t, S,
                  lambda: (2 * r(1, C) + 0.5).bfloat16(), {"gemv": 12, "gemv_glu": 0, "decode_attention": 3})


# ---------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------
@torch.no_grad()
def test_t5_decode_step(gpu):
    """``begin_decode`` over 37 encoder rows, then 10 steps, with the kernels on
    and off, each against ``decode_logits`` on the grown id list.  One eager step
    launches 5 L + 1 plain GEMVs, L gated ones and 2 L attentions."""
    from chiaswarm_amd.models.t5 import T5Config, T5Seq2Seq

    c = T5Config(vocab=1000, d_model=256, d_kv=64, heads=4, d_ff=512, layers=2)
    with torch.device(gpu):
        m = T5Seq2Seq(c, dec_layers=2).to(torch.bfloat16).eval().requires_grad_(False)
    init_random_fast_(m, seed=5)
    for blk in m.decoder.block:  # module docstring: T5 folds 1 / sqrt(d_kv) into q
        for a in (blk.layer[0].SelfAttention, blk.layer[1].EncDecAttention):
            a.q.weight.mul_(c.d_kv ** -0.5)
    prepare_model(m)
    gen = torch.Generator().manual_seed(6)
    enc = m.encode(torch.randn(1, 37, c.d_model, generator=gen).bfloat16().to(gpu))
    toks = [0] + torch.randint(2, c.vocab, (9,), generator=gen).tolist()
    refs = [m.decode_logits(enc, toks[:i + 1]).clone() for i in range(10)]
    L = len(m.decoder.block)
    steps = {}
    for on in (True, False):
        hip_ops.set_decode(on)
        try:
            m._graph = None  # a captured step keeps the kernels it was captured with
            m.new_cache(10, 37)
            m.begin_decode(enc)
            if on:
                before = dict(hip_ops.DECODE_STATS)
                m._decode_fn(torch.tensor([[toks[0]]], device=gpu), torch.tensor([0], device=gpu),
                             torch.tensor([1], dtype=torch.int32, device=gpu))
                assert _stats_delta(before) == {"gemv": 5 * L + 1, "gemv_glu": L, "decode_attention": 2 * L}
            steps[on] = [m.decode_step(toks[i], i).clone() for i in range(10)]
        finally:
            hip_ops.set_decode(True)
            m._graph = None
    for blk in m.decoder.block:
        a = blk.layer[0].SelfAttention
        ptr = a.w_fused.untyped_storage().data_ptr()
        assert all(p.weight.untyped_storage().data_ptr() == ptr for p in (a.q, a.k, a.v))
        assert a.w_fused.shape == (3 * c.heads * c.d_kv, c.d_model)
    for i in range(10):
        e = [rel_err(steps[True][i], refs[i]), rel_err(steps[False][i], refs[i]),
             rel_err(steps[True][i], steps[False][i])]
        print(f"t5 step {i}: rel_err on / off / on-off {e[0]:.3g} {e[1]:.3g} {e[2]:.3g}")
        assert steps[True][i].shape == (c.vocab,)
        assert max(e) < 3e-2, (i, e)


def _tiny_opt_d80(gpu):
    from chiaswarm_amd.models.blip2 import TINY_BLIP2, Blip2Captioner

    cfg = dataclasses.replace(TINY_BLIP2, lm_dim=320, lm_heads=4, lm_ffn=640, lm_depth=2, vocab=1000, max_pos=64)
    m = Blip2Captioner(cfg).eval().requires_grad_(False)
    init_random_fast_(m, seed=7)
    m = m.to(gpu).to(torch.bfloat16)
    prepare_model(m)
    return m


@torch.no_grad()
def test_opt_decode_step(gpu):
    """Prefill of a 20-row prefix and 4 ids, then 10 steps at head dim 80, with
    the kernels on and off, each against ``text_logits`` on the grown sequence.
    One eager step launches 4 L + 1 GEMVs and L attentions."""
    m = _tiny_opt_d80(gpu)
    assert m.lm[0].attn.dh == 80
    gen = torch.Generator().manual_seed(8)
    prefix = torch.randn(1, 20, 320, generator=gen).bfloat16().to(gpu)
    ids = [2] + torch.randint(3, 1000, (3,), generator=gen).tolist()
    toks = torch.randint(3, 1000, (10,), generator=gen).tolist()
    refs = [m.text_logits(prefix, ids + toks[:i + 1]).clone() for i in range(10)]
    L, n = len(m.lm), 20 + len(ids)
    steps = {}
    for on in (True, False):
        hip_ops.set_decode(on)
        try:
            m._graph = None  # a captured step keeps the kernels it was captured with
            m.new_cache(n + 10)
            assert rel_err(m.prefill(prefix, ids), m.text_logits(prefix, ids)) < 3e-2
            if on:
                before = dict(hip_ops.DECODE_STATS)
                m._decode_fn(torch.tensor([[toks[0]]], device=gpu), torch.tensor([n], device=gpu),
                             torch.tensor([n + 1], dtype=torch.int32, device=gpu))
                assert _stats_delta(before) == {"gemv": 4 * L + 1, "gemv_glu": 0, "decode_attention": L}
            steps[on] = [m.decode_step(toks[i], n + i).clone() for i in range(10)]
        finally:
            hip_ops.set_decode(True)
            m._graph = None
    for i in range(10):
        e = [rel_err(steps[True][i], refs[i]), rel_err(steps[False][i], refs[i]),
             rel_err(steps[True][i], steps[False][i])]
        print(f"opt step {i}: rel_err on / off / on-off {e[0]:.3g} {e[1]:.3g} {e[2]:.3g}")
        assert steps[True][i].shape == (1000,)
        assert max(e) < 3e-2, (i, e)


@pytest.mark.parametrize("lm", ["opt", "t5"])
@torch.no_grad()
def test_blip2_generate_uses_decode_kernels(gpu, lm):
    import numpy as np
    from PIL import Image

    from chiaswarm_amd.models.blip2 import TINY_BLIP2, Blip2Captioner
    from chiaswarm_amd.models.t5 import TINY_T5

    cfg = TINY_BLIP2 if lm == "opt" else dataclasses.replace(
        TINY_BLIP2, lm_type="t5", t5=TINY_T5, lm_dim=TINY_T5.d_model, vocab=TINY_T5.vocab, t5_dec_layers=2, bos_id=0,
        eos_id=1, pad_id=0)
    m = Blip2Captioner(cfg).eval().requires_grad_(False)
    init_random_fast_(m, seed=0)
    m = m.to(gpu).to(torch.bfloat16)
    prepare_model(m)
    img = Image.fromarray((np.random.default_rng(0).random((40, 48, 3)) * 255).astype(np.uint8))
    before = dict(hip_ops.DECODE_STATS)
    out = m.generate(img, [17, 42, 5], max_length=10)
    if lm == "opt":
        assert out[:3] == [17, 42, 5] and len(out) >= 5, "generation ended before a decode step ran"
    # (these geometries' head dim is 16: their decode attention takes the torch fallback, the GEMVs run the kernels)
    assert hip_ops.DECODE_STATS["gemv"] > before["gemv"], (before, hip_ops.DECODE_STATS)
    stats = dict(hip_ops.DECODE_STATS)
    m.generate(img, [17, 42, 5], max_length=10, use_cache=False)
    assert hip_ops.DECODE_STATS == stats, "the re-run loop launched a decode kernel"
