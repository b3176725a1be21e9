"""``ops.attention(..., bias=, kv_lens=)``: softmax(q k^T * scale + bias) v over
each sample's first ``kv_lens[b]`` keys.  CPU: the fp32 reference definition
(``ops._ref_attention_bias``, also the oracle of the GPU kernel tests) against
a hand-written per-sample loop, and the two model families routed through it
(T5's relative-position bias + key padding, XLM-R's batched forward)."""
import math

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models import t5 as t5_mod
from chiaswarm_amd.models.layers import init_random_, prepare_model
from chiaswarm_amd.models.t5 import TINY_T5, T5Encoder
from chiaswarm_amd.models.xlmr import TINY_XLMR, XLMRobertaSeries

B, H, SQ, SKV, D = 3, 2, 5, 7, 8
NEG = float("-inf")


def _qkv(sq=SQ, skv=SKV, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, sq, H, D, generator=g), torch.randn(B, skv, H, D, generator=g),
            torch.randn(B, skv, H, D, generator=g))


def _loop(q, k, v, scale, causal, bias, lens):
    """One (sample, head, query row) at a time, over the visible keys only."""
    b_, sq, h_, d_ = q.shape
    skv = k.shape[1]
    full = None if bias is None else bias.expand(b_, h_, sq, skv)
    o = torch.zeros(b_, sq, h_, d_)
    for b in range(b_):
        n = skv if lens is None else max(0, min(int(lens[b]), skv))
        for h in range(h_):
            for i in range(sq):
                keys = [j for j in range(n) if not causal or j <= i + (skv - sq)]
                if full is not None:
                    keys = [j for j in keys if full[b, h, i, j] != NEG]
                if not keys:
                    continue
                s = torch.stack([(q[b, i, h] * k[b, j, h]).sum() * scale + (0.0 if full is None else full[b, h, i, j])
                                 for j in keys])
                p = torch.softmax(s, 0)
                o[b, i, h] = sum(p[t] * v[b, j, h] for t, j in enumerate(keys))
    return o


def _bias(shape, seed=1):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 2


LENS = torch.tensor([SKV, 1, SKV // 2], dtype=torch.int32)


@pytest.mark.parametrize("case", ["bias", "lens", "both", "both_causal"])
def test_reference_matches_loop(case):
    q, k, v = _qkv()
    bias = _bias((B, H, SQ, SKV)) if case != "lens" else None
    lens = LENS if case != "bias" else None
    causal = case == "both_causal"
    scale = 1.0 / math.sqrt(D)
    got = ops.attention(q, k, v, scale, causal, bias=bias, kv_lens=lens)
    assert got.shape == (B, SQ, H, D) and got.is_contiguous()
    assert torch.allclose(got, _loop(q, k, v, scale, causal, bias, lens), atol=1e-5)
    assert torch.equal(got, ops._ref_attention_bias(q, k, v, scale, causal, bias, lens))


@pytest.mark.parametrize("shape", [(H, SQ, SKV), (B, 1, SQ, SKV), (1, 1, 1, SKV)])
def test_reference_broadcast_bias(shape):
    q, k, v = _qkv(seed=2)
    bias = _bias(shape, seed=3)
    got = ops.attention(q, k, v, 0.5, bias=bias, kv_lens=LENS)
    assert torch.allclose(got, _loop(q, k, v, 0.5, False, bias, LENS), atol=1e-5)


def test_reference_empty_rows_are_zero():
    q, k, v = _qkv(seed=4)
    bias = _bias((B, H, SQ, SKV), seed=5)
    bias[0, 1, 2] = NEG              # one row with every bias entry -inf
    bias[2, 0, 1, ::2] = NEG         # scattered -inf
    lens = torch.tensor([SKV, 0, SKV + 5], dtype=torch.int32)  # one empty sample, one that clips
    for causal in (False, True):
        got = ops.attention(q, k, v, 0.3, causal, bias=bias, kv_lens=lens)
        assert torch.isfinite(got).all()
        assert (got[1] == 0).all() and (got[0, 2, 1] == 0).all()
        assert got[0, 2, 0].abs().sum() > 0 and got[2].abs().sum() > 0
        assert torch.allclose(got, _loop(q, k, v, 0.3, causal, bias, lens), atol=1e-5)


def test_kv_len_with_kv_lens_raises():
    q, k, v = _qkv()
    with pytest.raises(ValueError):
        ops.attention(q, k, v, kv_len=torch.tensor([3], dtype=torch.int32), kv_lens=LENS)
    with pytest.raises(ValueError):
        ops.attention(q, k, v, kv_len=torch.tensor([3], dtype=torch.int32), bias=_bias((1, 1, 1, SKV)))


@pytest.mark.parametrize("causal", [False, True])
def test_plain_calls_unchanged(causal):
    q, k, v = _qkv(seed=6)
    scale = 1.0 / math.sqrt(D)
    want = ops._ref_attention(q, k, v, scale, causal)
    assert torch.equal(ops.attention(q, k, v, causal=causal), want)
    assert torch.equal(ops.attention(q, k, v, scale, causal, None, bias=None, kv_lens=None), want)
    n = torch.tensor([6], dtype=torch.int32)  # the KV-cache fill level: it moves the causal diagonal
    assert torch.equal(ops.attention(q, k, v, scale, causal, n), ops._ref_attention(q, k[:, :6], v[:, :6], scale, causal))


def test_t5_encoder_through_the_op(monkeypatch):
    enc = T5Encoder(TINY_T5)
    init_random_(enc, seed=11)
    prepare_model(enc)
    ids = torch.randint(2, TINY_T5.vocab, (3, 77), generator=torch.Generator().manual_seed(0))
    mask = torch.arange(77)[None, :] < torch.tensor([77, 1, 30])[:, None]
    want = enc(ids, mask)
    calls, op = [], ops.attention

    def spy(*a, **kw):
        calls.append(kw)
        return op(*a, **kw)

    monkeypatch.setattr(ops, "attention", spy)
    assert torch.equal(enc(ids, mask), want) and not calls  # the CPU path is today's formula
    monkeypatch.setattr(t5_mod, "FUSED_ATTENTION", True)
    got = enc(ids, mask)
    assert len(calls) == TINY_T5.layers and all(c["kv_lens"].tolist() == [77, 1, 30] for c in calls)
    assert torch.allclose(got, want, atol=1e-5), (got - want).abs().max()


@pytest.mark.parametrize("pre", [False, True])
def test_xlmr_batched_equals_per_row(pre):
    import dataclasses

    enc = XLMRobertaSeries(dataclasses.replace(TINY_XLMR, pre_transformation=pre))
    init_random_(enc, seed=12)
    prepare_model(enc)
    ids = torch.tensor([[0, 5, 17, 33, 2] + [1] * 10, [0, 9, 2] + [1] * 12, [0] + list(range(10, 23)) + [2]])
    with torch.no_grad():
        want = enc(ids)[0]
        got = enc.forward_batched(ids)[0]
    assert got.shape == want.shape
    assert torch.allclose(got, want, atol=2e-5, rtol=1e-4), (got - want).abs().max()
