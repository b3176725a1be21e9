"""KV-cached LLaMA decode on the CPU, where every op runs its torch
definition: ``ops.gemv(rms=)``, ``ops.gemv_glu``, ``ops.decode_attention`` with
``rope=`` and grouped K/V heads against references written out here, and a tiny
``LlamaLM`` (the geometry of tests/test_blip2_caption.py) whose prefill +
``decode_step`` must reproduce ``last_logits`` on the grown sequence.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import init_random_fast_, prepare_model
from chiaswarm_amd.models.llama import LlamaConfig, LlamaLM, RMSNorm

TINY = dict(vocab=100, dim=32, layers=2, heads=4, kv_heads=2, ffn=64)


def _r(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_gemv_rms_is_gemm_of_rmsnorm():
    x, w, res = _r(3, 40, seed=1), _r(24, 40, seed=2) / 6, _r(3, 24, seed=3)
    norm = RMSNorm(40, 1e-6)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * _r(40, seed=4))
        ref = ops.gemm(norm(x), w, None, residual=res, act="silu")
        y = ops.gemv(x, w, act="silu", residual=res, rms=(norm.weight, norm.eps))
    assert torch.allclose(y, ref, atol=1e-6, rtol=1e-6)
    out = torch.full((3, 30), -7.0)
    y2 = ops.gemv(x, w, act="silu", residual=res, rms=(norm.weight, norm.eps), out=out[:, 2:26])
    assert torch.equal(y2, y) and bool((out[:, :2] == -7).all()) and bool((out[:, 26:] == -7).all())
    # leading dims are kept
    assert ops.gemv(x.view(1, 3, 40), w, rms=(norm.weight.detach(), 1e-6)).shape == (1, 3, 24)


def test_gemv_glu_is_swiglu():
    x, wg, wu = _r(2, 40, seed=5), _r(24, 40, seed=6) / 6, _r(24, 40, seed=7) / 6
    y = ops.gemv_glu(x, wg, wu)
    assert torch.allclose(y, F.silu(x @ wg.t()) * (x @ wu.t()), atol=1e-6, rtol=1e-6)
    gamma = 1 + 0.2 * _r(40, seed=8)
    xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma
    y = ops.gemv_glu(x.view(1, 2, 40), wg, wu, act="gelu", rms=(gamma, 1e-5))
    assert y.shape == (1, 2, 24)
    assert torch.allclose(y[0], F.gelu(xn @ wg.t()) * (xn @ wu.t()), atol=1e-6, rtol=1e-6)
    with pytest.raises(ValueError):
        ops.gemv_glu(x, wg, wu, act="geglu")
    with pytest.raises(TypeError):
        ops.gemv_glu(x, wg, wu, bias=torch.zeros(24))  # no bias, no residual: not half-supported


def test_ln_and_rms_exclude_each_other():
    x, w = _r(1, 16), _r(8, 16)
    g = torch.ones(16)
    with pytest.raises(ValueError):
        ops.gemv(x, w, ln=(g, None, 1e-5), rms=(g, 1e-5))
    with pytest.raises(ValueError):
        ops.gemv_glu(x, w, w, ln=(g, None, 1e-5), rms=(g, 1e-5))


def _rope64(x, cos, sin):
    """rotate-half form in float64: x [..., D], cos / sin [D / 2]"""
    h = x.shape[-1] // 2
    a, b = x[..., :h].double(), x[..., h:].double()
    return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)


def test_decode_attention_rope_and_grouped_heads():
    B, H, Hkv, D, S, P = 2, 4, 2, 16, 12, 20
    q, kn, vn = _r(B, 1, H, D, seed=10), _r(B, 1, Hkv, D, seed=11), _r(B, 1, Hkv, D, seed=12)
    ang = torch.arange(P, dtype=torch.float64)[:, None] / (10000.0 ** (torch.arange(0, D, 2).double() / D))[None]
    cos, sin = ang.cos().float(), ang.sin().float()
    scale = 1.0 / math.sqrt(D)
    for n in (1, 5, S):
        for append in (True, False):
            kc, vc = _r(B, S, Hkv, D, seed=13), _r(B, S, Hkv, D, seed=14)
            k0, v0 = kc.clone(), vc.clone()
            kw = dict(k_new=kn, v_new=vn) if append else {}
            o = ops.decode_attention(q, kc, vc, scale, torch.tensor([n], dtype=torch.int32), rope=(cos, sin), **kw)
            c64, s64 = cos[n - 1].double(), sin[n - 1].double()
            fk, fv = k0.double().clone(), v0.double().clone()
            if append:
                fk[:, n - 1], fv[:, n - 1] = _rope64(kn[:, 0], c64, s64), vn[:, 0].double()
                assert torch.allclose(kc[:, n - 1].double(), fk[:, n - 1], atol=1e-6), "appended key is the rotated key"
                assert torch.equal(vc[:, n - 1], vn[:, 0])
            keep = torch.ones(S, dtype=torch.bool)
            keep[n - 1] = not append
            assert torch.equal(kc[:, keep], k0[:, keep]) and torch.equal(vc[:, keep], v0[:, keep])
            q64 = _rope64(q, c64, s64)
            ke, ve = fk[:, :n].repeat_interleave(H // Hkv, 2), fv[:, :n].repeat_interleave(H // Hkv, 2)
            p = torch.softmax(torch.einsum("bqhd,bshd->bhqs", q64, ke) * scale, -1)
            ref = torch.einsum("bhqs,bshd->bqhd", p, ve)
            assert o.shape == (B, 1, H, D)
            assert torch.allclose(o.double(), ref, atol=1e-5, rtol=1e-5), (n, append)
    kc, vc = _r(B, S, Hkv, D, seed=13), _r(B, S, Hkv, D, seed=14)
    k0 = kc.clone()
    o = ops.decode_attention(q, kc, vc, scale, torch.tensor([0], dtype=torch.int32), k_new=kn, v_new=vn,
                             rope=(cos, sin))
    assert not bool(o.any()) and torch.equal(kc, k0)
    with pytest.raises(ValueError):  # three K/V heads do not divide four query heads
        ops.decode_attention(q, _r(B, S, 3, D), _r(B, S, 3, D), scale, torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError):  # k_new carries the K/V head count
        ops.decode_attention(q, kc, vc, scale, torch.tensor([1], dtype=torch.int32), k_new=q, v_new=q)


def _tiny_lm(seed):
    m = LlamaLM(LlamaConfig(**TINY)).eval().requires_grad_(False)
    init_random_fast_(m, seed=seed)
    return m


@torch.no_grad()
def test_llama_decode_step_matches_last_logits():
    """Prefill of 6 embeddings, then 6 cached steps: each step's logits against
    ``last_logits`` on the grown sequence, atol = rtol = 1e-4 (the bound
    tests/test_blip2_caption.py holds ``last_logits`` to against transformers)."""
    m = _tiny_lm(3)
    names = list(m.state_dict().keys())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    prepare_model(m)
    assert list(m.state_dict().keys()) == names, "state-dict names changed"
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    for lyr in m.model.layers:
        a = lyr.self_attn
        ptr = a.w_qkv.untyped_storage().data_ptr()
        assert all(p.weight.untyped_storage().data_ptr() == ptr for p in (a.q_proj, a.k_proj, a.v_proj))
    seq = _r(1, 6, TINY["dim"], seed=20)
    assert torch.allclose(m.prefill(seq), m.last_logits(seq), atol=1e-4, rtol=1e-4)
    assert m.cache_capacity >= 12
    toks = [5, 17, 33, 2, 9, 60]
    for i, t in enumerate(toks):
        seq = torch.cat([seq, m.model.embed_tokens(torch.tensor([[t]]))], 1)
        got, ref = m.decode_step(t, 6 + i), m.last_logits(seq)
        assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), (i, float((got - ref).abs().max()))
    with pytest.raises(ValueError):
        m.decode_step(1, m.cache_capacity)
    # a model that was never prepared, or whose weights moved, builds the fused weight on demand
    m2 = _tiny_lm(3).double().float()
    m2.prefill(seq[:, :6])
    assert torch.allclose(m2.decode_step(toks[0], 6), m.last_logits(seq[:, :7]), atol=1e-4, rtol=1e-4)


def _tiny_instructblip(seed):
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
    init_random_fast_(m, seed=seed)
    return m


GENERATE_CASES = [(0, [17, 42, 5]), (1, [9]), (2, [60, 3, 3, 77, 21])]  # (seed, prompt ids)


@torch.no_grad()
def test_cached_generate_equals_rerun_loop():
    """The KV-cached ``generate`` returns the ids of the re-run loop for three
    prompts.  Token equality is not luck: with these seeds the smallest top-1 /
    top-2 logit gap over every step of the three generations is 3.3e-2 (printed
    below, and asserted to stay above 1e-3), two orders of magnitude above the
    1e-4 by which the cached logits may differ."""
    import numpy as np
    from PIL import Image

    img = Image.fromarray((np.random.default_rng(0).random((40, 48, 3)) * 255).astype(np.uint8))
    worst = float("inf")
    for seed, prompt in GENERATE_CASES:
        m = _tiny_instructblip(seed)
        qids = [3, 11, 25, 4]
        rerun = m.generate(img, prompt, max_length=9, qtext_ids=qids, use_cache=False)
        cached = m.generate(img, prompt, max_length=9, qtext_ids=qids)
        assert cached == rerun and len(cached) >= 1
        assert m.llama.cache is not None, "generate did not take the cached path"
        # the gaps of the re-run loop's logits
        emb = m.llama.model.embed_tokens
        prefix = m.image_prefix(m.preprocess(img), qids)
        ids = [m.cfg.bos_id] + prompt
        for t in rerun + [None]:
            top = m.llama.last_logits(torch.cat([prefix, emb(torch.tensor([ids]))], 1)).topk(2).values
            worst = min(worst, float(top[0] - top[1]))
            if t is not None:
                ids.append(t)
    print(f"smallest top-1 / top-2 gap: {worst:.3g}")
    assert worst > 1e-3
