"""CPU definitions of the distance-indexed score bias of ``ops.decode_attention``
(``rel_bias=``) and of the KV-cached decode of BLIP-2's two language models,
where every op runs its torch definition: ``T5Seq2Seq.begin_decode`` +
``decode_step`` against ``decode_logits`` on the grown id list, the OPT
``prefill`` + ``decode_step`` against ``text_logits``, and the cached
``generate`` against the re-run loop, on the tiny geometries of
tests/test_blip2_caption.py (atol = rtol = 1e-4, the figure that file holds the
same geometries to against transformers).
"""
import math

import pytest
import torch

from chiaswarm_amd import ops


def _r(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rope64(x, cos, sin):
    h = x.shape[-1] // 2
    a, b = x[..., :h].double(), x[..., h:].double()
    return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("B", [1, 2])
def test_decode_attention_rel_bias_is_the_explicit_softmax(B, H, Hkv):
    D, S, P = 16, 40, 43
    q, kn, vn = _r(B, 1, H, D, seed=10), _r(B, 1, Hkv, D, seed=11), _r(B, 1, Hkv, D, seed=12)
    rb = 3 * _r(H, P, seed=15)
    ang = torch.arange(P, dtype=torch.float64)[:, None] / (10000.0 ** (torch.arange(0, D, 2).double() / D))[None]
    cos, sin = ang.cos().float(), ang.sin().float()
    scale = 1.0 / math.sqrt(D)
    for n in (1, 2, 39, 40):
        for append in (False, True):
            for rope in (False, True):
                kc, vc = _r(B, S, Hkv, D, seed=13), _r(B, S, Hkv, D, seed=14)
                k0, v0 = kc.clone(), vc.clone()
                table = rb.clone()
                table[:, n:] = float("nan")  # distances the query cannot reach are never read
                kw = dict(k_new=kn, v_new=vn) if append else {}
                if rope:
                    kw["rope"] = (cos, sin)
                o = ops.decode_attention(q, kc, vc, scale, torch.tensor([n], dtype=torch.int32), rel_bias=table, **kw)
                c64, s64 = cos[n - 1].double(), sin[n - 1].double()
                fk, fv = k0.double().clone(), v0.double().clone()
                if append:
                    fk[:, n - 1] = _rope64(kn[:, 0], c64, s64) if rope else kn[:, 0].double()
                    fv[:, n - 1] = vn[:, 0].double()
                    assert torch.allclose(kc[:, n - 1].double(), fk[:, n - 1], atol=1e-6)
                    assert torch.equal(vc[:, n - 1], vn[:, 0])
                keep = torch.ones(S, dtype=torch.bool)
                keep[n - 1] = not append
                assert torch.equal(kc[:, keep], k0[:, keep]) and torch.equal(vc[:, keep], v0[:, keep])
                q64 = _rope64(q, c64, s64) if rope else q.double()
                ke, ve = fk[:, :n].repeat_interleave(H // Hkv, 2), fv[:, :n].repeat_interleave(H // Hkv, 2)
                s = torch.einsum("bqhd,bshd->bhqs", q64, ke) * scale
                s = s + rb[:, [n - 1 - j for j in range(n)]].double()[None, :, None]
                ref = torch.einsum("bhqs,bshd->bqhd", torch.softmax(s, -1), ve)
                assert o.shape == (B, 1, H, D)
                assert torch.allclose(o.double(), ref, atol=1e-5, rtol=1e-5), (n, append, rope)
    z = ops.decode_attention(q, kc, vc, scale, torch.tensor([0], dtype=torch.int32), rel_bias=rb)
    assert not bool(z.any())


def test_decode_attention_rel_bias_argument_errors():
    B, H, D, S = 1, 4, 16, 40
    q, kc, vc = _r(B, 1, H, D), _r(B, S, H, D, seed=1), _r(B, S, H, D, seed=2)
    len_t = torch.tensor([3], dtype=torch.int32)
    ops.decode_attention(q, kc, vc, 0.25, len_t, rel_bias=torch.zeros(H, S))
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.25, len_t, rel_bias=torch.zeros(H, S, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.25, len_t, rel_bias=torch.zeros(H + 1, S))
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.25, len_t, rel_bias=torch.zeros(H, S - 1))
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.25, len_t, rel_bias=torch.zeros(H, 2 * S)[:, ::2])
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, vc, 0.25, len_t, rel_bias=torch.zeros(H * S))


def _tiny(kind, tied=False):
    pytest.importorskip("transformers")
    from tests.test_blip2_caption import _hf_tiny, _hf_tiny_t5, _image, _ours

    hf_cfg, hf = _hf_tiny() if kind == "opt" else _hf_tiny_t5(tied)
    return _ours(hf_cfg, hf.state_dict()).requires_grad_(False), _image()


@pytest.mark.parametrize("tied", [False, True])
@torch.no_grad()
def test_t5_decode_step_matches_decode_logits(tied):
    m, img = _tiny("t5", tied)
    t5 = m.t5
    names = list(t5.state_dict().keys())
    before = {k: v.clone() for k, v in t5.state_dict().items()}
    enc = m.t5_encoder_states(m.image_prefix(m.preprocess(img)), [17, 42, 5])
    t5.new_cache(6, enc.shape[1])
    assert t5.cache_capacity >= 6 and t5.cache_capacity % 256 == 0
    bufs = [t.data_ptr() for kv in t5.cache for t in kv]
    t5.new_cache(3, 2)  # buffers that are large enough are kept
    assert [t.data_ptr() for kv in t5.cache for t in kv] == bufs
    t5.begin_decode(enc)
    ids = [0, 9, 33, 2, 60, 17]
    for i in range(6):
        got, ref = t5.decode_step(ids[i], i), t5.decode_logits(enc, ids[:i + 1])
        assert got.shape == ref.shape == (m.cfg.vocab,)
        assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), (i, float((got - ref).abs().max()))
    assert list(t5.state_dict().keys()) == names, "state-dict names changed"
    assert all(torch.equal(v, before[k]) for k, v in t5.state_dict().items())
    for blk in t5.decoder.block:  # the fused weights: no second resident copy
        a, e = blk.layer[0].SelfAttention, blk.layer[1].EncDecAttention
        ptr = a.w_fused.untyped_storage().data_ptr()
        assert all(p.weight.untyped_storage().data_ptr() == ptr for p in (a.q, a.k, a.v))
        ptr = e.w_fused.untyped_storage().data_ptr()
        assert all(p.weight.untyped_storage().data_ptr() == ptr for p in (e.k, e.v))
    with pytest.raises(ValueError):
        t5.decode_step(1, t5.cache_capacity)
    # a prefix mask shortens the encoder: the same logits as the truncated encoder states
    mask = torch.ones(1, enc.shape[1], dtype=torch.bool)
    mask[:, -2:] = False
    t5.begin_decode(enc, mask)
    got, ref = t5.decode_step(0, 0), t5.decode_logits(enc, [0], enc_mask=mask)
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4)
    # weights that moved: the fused weights and the distance table are rebuilt
    m2, _ = _tiny("t5", tied)
    t2 = m2.t5.double().float()
    t2.begin_decode(enc)
    assert torch.allclose(t2.decode_step(0, 0), t5.decode_logits(enc, [0]), atol=1e-4, rtol=1e-4)
    w = t2.decoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
    w.add_(0.5 * _r(*w.shape, seed=3))
    t2.begin_decode(enc)
    for i in range(3):
        got, ref = t2.decode_step(ids[i], i), t2.decode_logits(enc, ids[:i + 1])
        assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), i


@torch.no_grad()
def test_opt_decode_step_matches_text_logits():
    m, img = _tiny("opt")
    prefix = m.image_prefix(m.preprocess(img))
    ids = [2, 17, 42, 5]
    got, ref = m.prefill(prefix, ids), m.text_logits(prefix, ids)
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4)
    n = prefix.shape[1] + len(ids)
    assert m.cache_capacity >= n + 6
    for i, t in enumerate([9, 33, 2, 60, 17, 8]):
        ids.append(t)
        got, ref = m.decode_step(t, n + i), m.text_logits(prefix, ids)
        assert got.shape == ref.shape == (m.cfg.vocab,)
        assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), (i, float((got - ref).abs().max()))
    with pytest.raises(ValueError):
        m.decode_step(1, m.cfg.max_pos)


@pytest.mark.parametrize("kind,tied", [("t5", False), ("t5", True), ("opt", False)])
@torch.no_grad()
def test_cached_generate_equals_rerun_loop(kind, tied):
    """The cached ``generate`` returns the ids of the re-run loop.  The cached
    logits may differ from the re-run's by 1e-4; the smallest top-1 / top-2 gap
    of the re-run loop's logits over the generations is asserted to stay ten
    times above that."""
    m, img = _tiny(kind, tied)
    worst = float("inf")
    for prompt in ([17, 42, 5], [9], []):
        rerun = m.generate(img, prompt, max_length=10, use_cache=False)
        cached = m.generate(img, prompt, max_length=10, use_cache=True)
        assert cached == rerun and m.generate(img, prompt, max_length=10) == rerun
        assert (m.t5 if kind == "t5" else m).cache is not None, "generate did not take the cached path"
        px = m.image_prefix(m.preprocess(img))
        if kind == "t5":
            enc, ids = m.t5_encoder_states(px, prompt), [0]
            for t in rerun + [None]:
                top = m.t5.decode_logits(enc, ids).topk(2).values
                worst = min(worst, float(top[0] - top[1]))
                ids.append(t)
        else:
            ids = [2] + prompt
            for t in rerun[len(prompt):] + [None]:
                if len(ids) - 1 >= 9:  # max_length reached: no further logits were used
                    break
                top = m.text_logits(px, ids).topk(2).values
                worst = min(worst, float(top[0] - top[1]))
                ids.append(t)
    print(f"{kind} tied={tied}: smallest top-1 / top-2 gap {worst:.3g}")
    assert worst > 1e-3
