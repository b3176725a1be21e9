"""The bias / key-length attention kernel (csrc/kernels/attn_bias.hip) behind
``ops.attention(..., bias=, kv_lens=)`` against ``ops._ref_attention_bias`` on
the bf16-rounded inputs in fp32 on the CPU, and the model families wired to it
(run on the MI355X box: ``pytest -m gpu``).

Rows that must be zeros (no visible key) are compared for exact zeros and left
out of the norm; every case keeps them to at most one sample."""
import copy
import math

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import init_random_, prepare_model
from chiaswarm_amd.ops import hip_ops

pytestmark = pytest.mark.gpu

B, H = 3, 2
NEG = float("-inf")
LIMIT = 1.5e-2  # the limit of every attention kernel in tests/test_kernels_gpu.py


@pytest.fixture
def waves():
    yield hip_ops.set_attn_bias_waves
    hip_ops.set_attn_bias_waves(0)


def _qkv(Sq, Skv, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, s, H, D, generator=g).to(torch.bfloat16) for s in (Sq, Skv, Skv))


def _bias(shape, Skv, seed=1, inf_row=True):
    """std-4 bias with scattered -inf (never on key 0, so a sample cut to one
    key keeps it), one column spiked by +30 in the last key block (forces an
    online-softmax rescale there) and, in sample 0 only, one all -inf row."""
    g = torch.Generator().manual_seed(seed)
    bias = torch.randn(*shape, generator=g) * 4
    hole = torch.rand(*shape, generator=g) < 0.1
    hole[..., 0] = False
    bias = bias.masked_fill(hole, NEG)
    bias[..., Skv - 1] = bias[..., Skv - 1].nan_to_num(neginf=0.0) + 30
    if inf_row and len(shape) == 4 and shape[0] == B and shape[2] > 1:
        bias[0, -1, shape[2] // 2] = NEG
    return bias


def _check(q, k, v, scale, causal, bias, lens, got, max_zero_samples=1):
    Sq, Skv = q.shape[1], k.shape[1]
    ref = ops._ref_attention_bias(q.float(), k.float(), v.float(), scale, causal, bias, lens)
    vis = torch.ones(B, H, Sq, Skv, dtype=torch.bool)
    if lens is not None:
        vis &= (torch.arange(Skv)[None, :] < lens.long()[:, None])[:, None, None, :]
    if causal:
        vis &= ~torch.ones(Sq, Skv, dtype=torch.bool).triu(1 + Skv - Sq)
    if bias is not None:
        vis &= bias.expand(B, H, Sq, Skv) != NEG
    zero = ~vis.any(-1).permute(0, 2, 1)  # [B, Sq, H]
    assert int(zero.flatten(1).any(1).sum()) <= max_zero_samples
    got = got.float().cpu()
    assert torch.isfinite(got).all()
    assert (got[zero] == 0).all() and (ref[zero] == 0).all()
    err = ((got - ref)[~zero].norm() / (ref[~zero].norm() + 1e-12)).item()
    print(f"rel_err {err:.3e} zero_rows {int(zero.sum())}")
    assert err < LIMIT


def _run(gpu, q, k, v, scale, causal, bias, lens):
    return ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), scale, causal,
                         bias=None if bias is None else bias.to(gpu), kv_lens=None if lens is None else lens.to(gpu))


@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("D", [16, 40, 64, 128])
@pytest.mark.parametrize("Sq", [1, 77, 200])
@pytest.mark.parametrize("Skv", [64, 65, 77, 130])
def test_bias_and_lens(gpu, waves, Skv, Sq, D, nw):
    waves(nw)
    q, k, v = _qkv(Sq, Skv, D)
    bias = _bias((B, H, Sq, Skv), Skv)
    lens = torch.tensor([Skv, 1, Skv // 2], dtype=torch.int32)
    scale = 1 / math.sqrt(D)
    _check(q, k, v, scale, False, bias, lens, _run(gpu, q, k, v, scale, False, bias, lens))


@pytest.mark.parametrize("shape", [(B, H, 77, 77), (H, 77, 77), (B, 1, 77, 77), (1, 1, 1, 77)])
@pytest.mark.parametrize("use_lens", [False, True])
def test_broadcast_bias(gpu, shape, use_lens):
    q, k, v = _qkv(77, 77, 64, seed=2)
    bias = _bias(shape, 77, seed=3)
    lens = torch.tensor([77, 1, 38], dtype=torch.int32) if use_lens else None
    _check(q, k, v, 0.125, False, bias, lens, _run(gpu, q, k, v, 0.125, False, bias, lens))


@pytest.mark.parametrize("lens", [[77, 0, 38], [86, 1, 38], [130, 64, 65]])
@pytest.mark.parametrize("with_bias", [False, True])
def test_lens_zero_and_clip(gpu, lens, with_bias):
    Skv = 130 if lens[0] == 130 else 77
    q, k, v = _qkv(77, Skv, 64, seed=4)
    bias = _bias((B, H, 77, Skv), Skv, seed=5, inf_row=False) if with_bias else None
    lens = torch.tensor(lens, dtype=torch.int32)
    _check(q, k, v, 0.125, False, bias, lens, _run(gpu, q, k, v, 0.125, False, bias, lens))


def test_padding_keys_need_not_be_finite(gpu):
    """Keys / values past kv_lens[b] are never read (a padded batch may hold anything there)."""
    q, k, v = _qkv(77, 77, 64, seed=6)
    lens = torch.tensor([77, 5, 38], dtype=torch.int32)
    kg, vg = k.clone(), v.clone()
    kg[1, 5:], vg[1, 5:], kg[2, 38:], vg[2, 38:] = float("nan"), float("inf"), float("inf"), float("nan")
    _check(q, k, v, 0.125, False, None, lens, _run(gpu, q, kg, vg, 0.125, False, None, lens))


@pytest.mark.parametrize("nw", [1, 4])
@pytest.mark.parametrize("Sq,Skv", [(33, 77), (77, 77), (130, 130), (1, 65)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_causal_with_lens(gpu, waves, Sq, Skv, with_bias, nw):
    """The causal diagonal is aligned against the tensor's Skv, not the clipped length."""
    waves(nw)
    q, k, v = _qkv(Sq, Skv, 64, seed=7)
    bias = _bias((H, Sq, Skv), Skv, seed=8) if with_bias else None
    lens = torch.tensor([Skv, 1, Skv // 2], dtype=torch.int32)
    _check(q, k, v, 0.125, True, bias, lens, _run(gpu, q, k, v, 0.125, True, bias, lens))


def test_fused_qkv_strided_views(gpu):
    S, D = 77, 64
    qkv = torch.randn(B, S, 3, H, D, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    bias = _bias((B, H, S, S), S, seed=10)
    lens = torch.tensor([S, 1, S // 2], dtype=torch.int32)
    g = qkv.to(gpu)
    got = ops.attention(g[:, :, 0], g[:, :, 1], g[:, :, 2], 0.125, bias=bias.to(gpu), kv_lens=lens.to(gpu))
    assert got.shape == (B, S, H, D) and got.is_contiguous()
    _check(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0.125, False, bias, lens, got)


def test_unaligned_bias_rows_and_batch_strides(gpu):
    """A bias that is a view into a larger buffer: q stride 81 (not a multiple of 4), base offset 3 floats."""
    S = 77
    q, k, v = _qkv(S, S, 64, seed=11)
    bias = _bias((B, H, S, S), S, seed=12)
    buf = torch.zeros(3 + B * H * S * 81, device=gpu)
    view = buf[3:].view(B, H, S, 81)[..., :S]
    view.copy_(bias)
    assert view.stride() == (H * S * 81, S * 81, 81, 1)
    got = ops.attention(q.to(gpu), k.to(gpu), v.to(gpu), 0.125, bias=view)
    _check(q, k, v, 0.125, False, bias, None, got)


def test_wrapper_validation_and_fallback(gpu):
    q, k, v = (t.to(gpu) for t in _qkv(5, 7, 16))
    with pytest.raises(TypeError):
        ops.attention(q, k, v, bias=torch.zeros(7, device=gpu, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        ops.attention(q, k, v, kv_lens=torch.ones(B, device=gpu, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.attention(q.float(), k.float(), v.float(), kv_lens=torch.ones(B, device=gpu, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.attention(q, k, v, bias=torch.zeros(B, H, 5, 6, device=gpu))
    with pytest.raises(ValueError):
        ops.attention(q, k, v, kv_lens=torch.ones(B + 1, device=gpu, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.attention(q, k, v, kv_len=torch.ones(1, device=gpu, dtype=torch.int32),
                      kv_lens=torch.ones(B, device=gpu, dtype=torch.int32))
    # head dims the kernel does not take run the reference formula on the device
    g = torch.Generator().manual_seed(13)
    for D in (12, 136):
        q, k, v = (torch.randn(B, s, H, D, generator=g).to(torch.bfloat16) for s in (5, 7, 7))
        lens = torch.tensor([7, 1, 3], dtype=torch.int32)
        bias = _bias((H, 5, 7), 7, seed=14)
        _check(q, k, v, 0.2, False, bias, lens, _run(gpu, q, k, v, 0.2, False, bias, lens))


def test_graph_replay_follows_new_contents(gpu):
    S = 77
    q, k, v = _qkv(S, S, 64, seed=15)
    bias = _bias((H, S, S), S, seed=16)
    lens = torch.tensor([S, 1, S // 2], dtype=torch.int32)
    qg, kg, vg, bg, lg = (t.to(gpu) for t in (q, k, v, bias, lens))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention(qg, kg, vg, 0.125, bias=bg, kv_lens=lg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention(qg, kg, vg, 0.125, bias=bg, kv_lens=lg)
    graph.replay()
    _check(q, k, v, 0.125, False, bias, lens, out)
    bias2 = _bias((H, S, S), S, seed=17)
    lens2 = torch.tensor([9, S, 70], dtype=torch.int32)
    bg.copy_(bias2)
    lg.copy_(lens2)
    graph.replay()
    _check(q, k, v, 0.125, False, bias2, lens2, out)


def _rel(got, ref):
    return ((got.float().cpu() - ref).norm() / ref.norm()).item()


def test_t5_encoder_gpu_matches_fp32(gpu):
    from chiaswarm_amd.models.t5 import TINY_T5, T5Encoder

    cpu = T5Encoder(TINY_T5)
    init_random_(cpu, seed=21)
    prepare_model(cpu)
    g = copy.deepcopy(cpu).to(gpu).to(torch.bfloat16)
    prepare_model(g)
    ids = torch.randint(2, TINY_T5.vocab, (3, 77), generator=torch.Generator().manual_seed(0))
    mask = torch.arange(77)[None, :] < torch.tensor([77, 1, 30])[:, None]
    calls, op = [], ops.attention
    try:
        ops.attention = lambda *a, **kw: (calls.append(kw), op(*a, **kw))[1]
        got = g(ids.to(gpu), mask.to(gpu))
    finally:
        ops.attention = op
    assert len(calls) == TINY_T5.layers and all(c["bias"] is not None and c["kv_lens"] is not None for c in calls)
    ref = cpu(ids, mask)
    # rows past each sample's length attend to the same keys on both paths: the whole tensor is compared
    err = _rel(got, ref)
    print(f"rel_err {err:.3e}")
    assert err < 3e-2  # the figure of test_blip2_gpu_matches_fp32


def test_flan_t5_decode_logits_gpu_matches_fp32(gpu):
    from chiaswarm_amd.models.t5 import TINY_T5, T5Seq2Seq

    cpu = T5Seq2Seq(TINY_T5, dec_layers=2)
    init_random_(cpu, seed=22)
    prepare_model(cpu)
    g = copy.deepcopy(cpu).to(gpu).to(torch.bfloat16)
    prepare_model(g)
    x = torch.randn(1, 40, TINY_T5.d_model, generator=torch.Generator().manual_seed(1))
    mask = (torch.arange(40) < 29)[None]
    ids = [0, 9, 33, 17, 5]
    ref = cpu.decode_logits(cpu.encode(x, mask), ids, mask)
    got = g.decode_logits(g.encode(x.to(gpu).to(torch.bfloat16), mask.to(gpu)), ids, mask.to(gpu))
    err = _rel(got, ref)
    print(f"rel_err {err:.3e}")
    assert err < 3e-2


def test_xlmr_batched_gpu_matches_fp32(gpu):
    from chiaswarm_amd.models.xlmr import TINY_XLMR, XLMRobertaSeries

    cpu = XLMRobertaSeries(TINY_XLMR)
    init_random_(cpu, seed=23)
    prepare_model(cpu)
    g = copy.deepcopy(cpu).to(gpu).to(torch.bfloat16)
    prepare_model(g)
    ids = torch.tensor([[0, 5, 17, 33, 2] + [1] * 10, [0, 9, 2] + [1] * 12, [0] + list(range(10, 23)) + [2]])
    assert (ids != 1).sum(1).tolist() == [5, 3, 15]
    with torch.no_grad():
        ref = cpu(ids)[0]
        got = g(ids.to(gpu))[0]
    err = _rel(got, ref)
    print(f"rel_err {err:.3e}")
    assert err < 2e-2  # the figure of test_altdiffusion_on_gpu


def test_altdiffusion_text_encoding_is_graphed(gpu):
    from chiaswarm_amd.pipelines.sd import StableDiffusion

    pipe = StableDiffusion("tiny-alt", device=gpu, seed=2)
    assert pipe.use_graphs
    prompts, negatives = ["ein Hund im Park", "un chat noir sur un toit"], ["", "blurry"]
    def flat(x):
        return [x.clone()] if torch.is_tensor(x) else [t for y in x for t in flat(y)]

    ctx1, _, kv1 = pipe.encode(prompts, negatives, True)
    ctx1, kv1 = ctx1.clone(), flat(kv1)
    ctx2, _, kv2 = pipe.encode(prompts, negatives, True)
    assert hasattr(pipe, "_text_graphs")
    assert torch.isfinite(ctx2.float()).all()
    assert torch.equal(ctx1, ctx2) and kv1 and all(torch.equal(a, b) for a, b in zip(kv1, flat(kv2)))
    # a replay with other prompts (other row lengths) follows them
    other = ["a photograph of an astronaut riding a horse on the moon", "ein Hund"]
    ctx3 = pipe.encode(other, negatives, True)[0].clone()
    eager, _, _ = pipe._text_fn(tuple(tok(negatives + other).to(gpu) for tok in pipe.tokenizers))
    assert not torch.equal(ctx3, ctx1) and _rel(ctx3, eager.float().cpu()) < 1e-3
