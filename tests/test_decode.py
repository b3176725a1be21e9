"""CPU definitions of the decode ops (``ops.gemv``, ``ops.decode_attention``)
and Bark's decode step wired to them: each must equal, bit for bit, the
composition of existing ops it replaces."""
import math

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models import bark as bk
from chiaswarm_amd.models.layers import init_random_fast_, prepare_model


@pytest.mark.parametrize("m", [1, 3, 9])
@pytest.mark.parametrize("use_ln", [False, True])
@pytest.mark.parametrize("act", [None, "gelu", "silu", "quick_gelu", "relu"])
@pytest.mark.parametrize("extras", [False, True])
def test_gemv_is_layer_norm_plus_gemm(m, use_ln, act, extras):
    torch.manual_seed(0)
    k, n = 40, 24
    x = torch.randn(2, m, k) * 2 + 0.5
    w = torch.randn(n, k) / math.sqrt(k)
    bias = torch.randn(n) if extras else None
    res = torch.randn(2, m, n) if extras else None
    gamma, beta = torch.rand(k) + 0.5, torch.randn(k)
    ln = (gamma, beta if extras else None, 1e-5) if use_ln else None
    y = ops.gemv(x, w, bias, act=act, residual=res, ln=ln)
    xn = ops.layer_norm(x, ln[0], ln[1], ln[2]) if use_ln else x
    ref = ops.gemm(xn, w, bias, residual=res, act=act)
    assert y.shape == (2, m, n)
    assert torch.equal(y, ref)


def test_gemv_out_view():
    torch.manual_seed(1)
    x, w = torch.randn(3, 16), torch.randn(10, 16)
    buf = torch.full((5, 14), 7.0)
    y = ops.gemv(x, w, out=buf[1:4, 2:12])
    assert torch.equal(y, ops.gemm(x, w))
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:4, 2:12] = False
    assert (buf[keep] == 7.0).all()


def _cache_case(b=2, s=12, h=3, d=8):
    torch.manual_seed(2)
    q, kn, vn = (torch.randn(b, 1, h, d) for _ in range(3))
    kc, vc = torch.randn(b, s, h, d), torch.randn(b, s, h, d)
    return q, kc, vc, kn, vn


@pytest.mark.parametrize("n", [1, 5, 12])
def test_decode_attention_append_is_index_copy_plus_attention(n):
    q, kc, vc, kn, vn = _cache_case()
    kc2, vc2 = kc.clone(), vc.clone()
    len_t = torch.tensor([n], dtype=torch.int32)
    scale = 1.0 / math.sqrt(q.shape[-1])
    o = ops.decode_attention(q, kc, vc, scale, len_t, k_new=kn, v_new=vn)
    pos_t = torch.tensor([n - 1])
    kc2.index_copy_(1, pos_t, kn)
    vc2.index_copy_(1, pos_t, vn)
    ref = ops.attention(q, kc2, vc2, scale, kv_len=len_t)
    assert o.shape == q.shape
    assert torch.equal(o, ref)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert torch.equal(kc[:, n - 1], kn[:, 0]) and torch.equal(vc[:, n - 1], vn[:, 0])


def test_decode_attention_without_append_and_empty():
    q, kc, vc, _, _ = _cache_case()
    kc0 = kc.clone()
    len_t = torch.tensor([7], dtype=torch.int32)
    o = ops.decode_attention(q, kc, vc, 0.3, len_t)
    assert torch.equal(o, ops.attention(q, kc, vc, 0.3, kv_len=len_t))
    assert torch.equal(kc, kc0)
    z = ops.decode_attention(q, kc, vc, 0.3, torch.tensor([0], dtype=torch.int32))
    assert z.shape == q.shape and not z.any()


def test_decode_attention_argument_errors():
    q, kc, vc, kn, vn = _cache_case()
    with pytest.raises(TypeError):
        ops.decode_attention(q, kc, vc, 0.3, torch.tensor([3]))  # int64
    with pytest.raises(TypeError):
        ops.decode_attention(q, kc, vc, 0.3, 3)
    len_t = torch.tensor([3], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.3, len_t, k_new=kn[:, :, :2], v_new=vn)
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.3, len_t, k_new=kn)
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc[:, :, :2], vc, 0.3, len_t)


def _old_decode(m, ids, pos_t, len_t):
    """The decode step as it was composed before ops.gemv / ops.decode_attention"""
    x = m.input_embeds_layer(ids) + m.position_embeds_layer.weight.index_select(0, pos_t)[None]
    x = x.to(m.lm_head.weight.dtype)
    for i, layer in enumerate(m.layers):
        at = layer.attn
        b = x.shape[0]
        qkv = at.att_proj(layer.layernorm_1(x)).view(b, 1, 3, at.nh, at.dh)
        kc, vc = m.cache[i]
        kc.index_copy_(1, pos_t, qkv[:, :, 1])
        vc.index_copy_(1, pos_t, qkv[:, :, 2])
        o = ops.attention(qkv[:, :, 0], kc, vc, 1.0 / math.sqrt(at.dh), kv_len=len_t)
        x = at.out_proj(o.reshape(b, 1, -1), residual=x)
        x = layer.mlp.out_proj(layer.mlp.in_proj(layer.layernorm_2(x), act="gelu"), residual=x)
    return m.lm_head(m.layernorm_final(x[:, -1])).float()


@torch.no_grad()
def test_bark_tiny_decode_matches_old_composition():
    sc, _, _ = bk.bark_configs("tiny")
    m = bk.BarkCausalGPT(sc).eval().requires_grad_(False)
    init_random_fast_(m, seed=5)
    prepare_model(m)
    torch.manual_seed(3)
    ids = torch.randint(0, 10000, (1, 12))
    m.new_cache()
    m(ids[:, :8], pos=0)
    new = [m.decode_step(int(ids[0, i]), i).clone() for i in range(8, 12)]
    m._kv = None
    m.new_cache()
    m(ids[:, :8], pos=0)
    for j, i in enumerate(range(8, 12)):
        old = _old_decode(m, ids[:, i:i + 1], torch.tensor([i]), torch.tensor([i + 1], dtype=torch.int32))
        assert torch.equal(new[j], old), i
