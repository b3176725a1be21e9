"""T5 v1.1 encoder (DeepFloyd IF text encoder, T5-XXL: 24 layers, d_model
4096, 64 heads, gated-GELU FFN 10240) with the transformers parameter names
(``shared``, ``encoder.block.{i}.layer.{0,1}...``), so an IF
``text_encoder/*.safetensors`` loads without renames.  Reached by the
reference via ``stage_1.encode_prompt`` (swarm/diffusion/diffusion_func_if.py:43-45).

MI355X path: Q/K/V/O and the gated FFN are MFMA GEMMs (tanh-GELU of wi_0
fused into its epilogue, the residual adds fused into wo / o).  The attention
core (77 tokens, per-head relative-position bias, key-padding mask) is one
launch of the bias / key-length attention kernel (``ops.attention(..., bias=,
kv_lens=)``, csrc/kernels/attn_bias.hip) on [B, S, H, D] views of the
projections: the fp32 bias is added to the unscaled scores in the kernel and
the padding mask travels as per-sample key counts.  CPU tensors keep the plain
fp32 torch formula (the transformers-parity tests run there).

``T5Seq2Seq`` greedy decode is KV-cached: ``begin_decode`` projects every
decoder layer's cross-attention K/V of the encoder output once, ``decode_step``
runs one token through the decode kernels (``ops.gemv`` / ``ops.gemv_glu`` with
the RMSNorm prologues, ``ops.decode_attention`` with the self-attention append
and the relative-position bias as a distance-indexed table), eight launches a
layer, replayed from one hipGraph.  ``decode_logits`` re-runs a whole prefix
without a cache (the A/B of tools/captiondecodebench.py).
"""
from __future__ import annotations

import dataclasses
import hashlib
import math
import os

import torch
import torch.nn as nn

from .. import ops
from .layers import Linear

# None: the fused attention op for bf16 tensors on the HIP path, the torch
# formula elsewhere.  True / False force one of them (tests: the op's fp32
# reference definition against the formula on the CPU).
FUSED_ATTENTION: bool | None = None


def _fused(x: torch.Tensor) -> bool:
    if FUSED_ATTENTION is not None:
        return FUSED_ATTENTION
    return ops.use_hip(x) and x.dtype == torch.bfloat16


def key_lens(mask: torch.Tensor | None):
    """Key-padding mask [B, S] (bool) -> per-sample key counts (int32 [B]) for
    the attention op, computed on the mask's device with no host read.
    ``T5Tokenizer`` (and BLIP-2's query-prefix + prompt layout) only produce
    PREFIX masks (ones, then zeros), for which "the first n keys" is the mask
    exactly; a mask with holes is not representable this way."""
    return None if mask is None else mask.sum(1).to(torch.int32)


@dataclasses.dataclass
class T5Config:
    vocab: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    heads: int = 64
    d_ff: int = 10240
    layers: int = 24
    buckets: int = 32
    max_distance: int = 128
    eps: float = 1e-6


T5_XXL = T5Config()
TINY_T5 = T5Config(vocab=1000, d_model=64, d_kv=16, heads=4, d_ff=128, layers=2)


class T5RMSNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.eps = eps

    def forward(self, x):
        xf = x.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)
        return (y * self.weight.float()).to(x.dtype)


def relative_position_bucket(rel: torch.Tensor, num_buckets=32, max_distance=128, bidirectional=True) -> torch.Tensor:
    """T5 bucketing of (key - query) offsets; the decoder's self-attention is
    unidirectional (only offsets <= 0, all buckets for the past)."""
    if bidirectional:
        num_buckets //= 2
        out = (rel > 0).long() * num_buckets
        n = rel.abs()
    else:
        out = torch.zeros_like(rel)
        n = (-rel).clamp_min(0)
    max_exact = num_buckets // 2
    large = max_exact + (torch.log(n.float().clamp_min(1) / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).long()
    large = large.clamp_max(num_buckets - 1)
    return out + torch.where(n < max_exact, n, large)


class _SelfAttention(nn.Module):
    def __init__(self, c: T5Config, has_bias: bool):
        super().__init__()
        inner = c.heads * c.d_kv
        self.c = c
        self.q = Linear(c.d_model, inner, bias=False)
        self.k = Linear(c.d_model, inner, bias=False)
        self.v = Linear(c.d_model, inner, bias=False)
        self.o = Linear(inner, c.d_model, bias=False)
        if has_bias:
            self.relative_attention_bias = nn.Embedding(c.buckets, c.heads)

    def fuse(self, names):
        """One weight for the projections ``names`` (decoder self-attention:
        q, k, v for the decode step's GEMV; cross-attention: k, v for the
        one-off encoder projection); their weights become row-range views of it
        (models/llama.py ``_Attn.prepare``), so nothing is resident twice and
        state-dict names do not change.  Rebuilt if the parameters moved
        (device, dtype or storage); returns (weight, rebuilt)."""
        projs = [getattr(self, n) for n in names]
        w, p0 = getattr(self, "w_fused", None), projs[0].weight
        if (w is not None and w.device == p0.device and w.dtype == p0.dtype
                and all(p.weight.untyped_storage().data_ptr() == w.untyped_storage().data_ptr() for p in projs)):
            return w, False
        w = torch.cat([p.weight.detach() for p in projs], 0)
        r = 0
        for p in projs:
            n = p.weight.shape[0]
            p.weight.data = w[r:r + n]
            r += n
        self.w_fused = w
        return w, True

    def position_bias(self, s, device, bidirectional=True):
        pos = torch.arange(s, device=device)
        rel = pos[None, :] - pos[:, None]
        bucket = relative_position_bucket(rel, self.c.buckets, self.c.max_distance, bidirectional)
        return self.relative_attention_bias(bucket).permute(2, 0, 1).float()  # [H, S, S]


class _AttnLayer(nn.Module):
    def __init__(self, c, has_bias):
        super().__init__()
        self.SelfAttention = _SelfAttention(c, has_bias)
        self.layer_norm = T5RMSNorm(c.d_model, c.eps)

    def forward(self, x, bias, mask, lens=None):
        a = self.SelfAttention
        b, s, _ = x.shape
        h = self.layer_norm(x)
        if _fused(x):  # lens = key_lens(mask), computed once per forward by the caller
            q, k, v = (m(h).view(b, s, a.c.heads, a.c.d_kv) for m in (a.q, a.k, a.v))
            o = ops.attention(q, k, v, 1.0, bias=bias, kv_lens=lens)  # T5: no 1/sqrt(d) scaling
            return a.o(o.reshape(b, s, -1), residual=x)
        q, k, v = (m(h).view(b, s, a.c.heads, a.c.d_kv).transpose(1, 2).float() for m in (a.q, a.k, a.v))
        scores = q @ k.transpose(-1, -2) + bias[None]  # T5: no 1/sqrt(d) scaling
        if mask is not None:
            scores = scores.masked_fill(~mask[:, None, None, :], float("-inf"))
        o = (torch.softmax(scores, -1) @ v).transpose(1, 2).reshape(b, s, -1).to(x.dtype)
        return a.o(o, residual=x)


class _FFLayer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.DenseReluDense = nn.Module()
        self.DenseReluDense.wi_0 = Linear(c.d_model, c.d_ff, bias=False)
        self.DenseReluDense.wi_1 = Linear(c.d_model, c.d_ff, bias=False)
        self.DenseReluDense.wo = Linear(c.d_ff, c.d_model, bias=False)
        self.layer_norm = T5RMSNorm(c.d_model, c.eps)

    def forward(self, x):
        d = self.DenseReluDense
        h = self.layer_norm(x)
        g = d.wi_0(h, act="gelu_tanh")
        return d.wo(g * d.wi_1(h), residual=x)


class _Block(nn.Module):
    def __init__(self, c, has_bias):
        super().__init__()
        self.layer = nn.ModuleList([_AttnLayer(c, has_bias), _FFLayer(c)])


class T5Encoder(nn.Module):
    def __init__(self, c: T5Config = T5_XXL):
        super().__init__()
        self.cfg = c
        self.shared = nn.Embedding(c.vocab, c.d_model)
        self.encoder = nn.Module()
        self.encoder.block = nn.ModuleList([_Block(c, i == 0) for i in range(c.layers)])
        self.encoder.final_layer_norm = T5RMSNorm(c.d_model, c.eps)
        self.checkpoint_ignore = ("encoder.embed_tokens.",)  # tied to ``shared`` in transformers checkpoints

    @torch.no_grad()
    def forward(self, ids: torch.Tensor, mask: torch.Tensor | None = None) -> torch.Tensor:
        dt = self.shared.weight.dtype
        x = self.shared(ids).to(dt)
        bias = self.encoder.block[0].layer[0].SelfAttention.position_bias(ids.shape[1], ids.device)
        lens = None
        if _fused(x):
            bias, lens = bias.contiguous(), key_lens(mask)
        for blk in self.encoder.block:
            x = blk.layer[0](x, bias, mask, lens)
            x = blk.layer[1](x)
        return self.encoder.final_layer_norm(x)


def _attend(a: "_SelfAttention", h, kv_src, bias, mask, lens=None):
    """softmax(q k^T + bias [+ key mask]) v for one T5 attention (no 1/sqrt(d)).
    ``lens`` = key_lens(mask), used by the fused op in place of the mask."""
    b, s, _ = h.shape
    t = kv_src.shape[1]
    if _fused(h):
        q = a.q(h).view(b, s, a.c.heads, a.c.d_kv)
        k = a.k(kv_src).view(b, t, a.c.heads, a.c.d_kv)
        v = a.v(kv_src).view(b, t, a.c.heads, a.c.d_kv)
        return ops.attention(q, k, v, 1.0, bias=bias, kv_lens=lens).reshape(b, s, -1)
    q = a.q(h).view(b, s, a.c.heads, a.c.d_kv).transpose(1, 2).float()
    k = a.k(kv_src).view(b, t, a.c.heads, a.c.d_kv).transpose(1, 2).float()
    v = a.v(kv_src).view(b, t, a.c.heads, a.c.d_kv).transpose(1, 2).float()
    scores = q @ k.transpose(-1, -2)
    if bias is not None:
        scores = scores + bias[None]
    if mask is not None:
        scores = scores.masked_fill(~mask[:, None, None, :], float("-inf"))
    return (torch.softmax(scores, -1) @ v).transpose(1, 2).reshape(b, s, -1)


class _DecSelfLayer(nn.Module):
    def __init__(self, c, has_bias):
        super().__init__()
        self.SelfAttention = _SelfAttention(c, has_bias)
        self.layer_norm = T5RMSNorm(c.d_model, c.eps)

    def forward(self, x, bias):
        h = self.layer_norm(x)
        return self.SelfAttention.o(_attend(self.SelfAttention, h, h, bias, None).to(x.dtype), residual=x)


class _CrossLayer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.EncDecAttention = _SelfAttention(c, False)
        self.layer_norm = T5RMSNorm(c.d_model, c.eps)

    def forward(self, x, enc, enc_mask, enc_lens=None):
        h = self.layer_norm(x)
        return self.EncDecAttention.o(_attend(self.EncDecAttention, h, enc, None, enc_mask, enc_lens).to(x.dtype),
                                      residual=x)


class _DecBlock(nn.Module):
    def __init__(self, c, has_bias):
        super().__init__()
        self.layer = nn.ModuleList([_DecSelfLayer(c, has_bias), _CrossLayer(c), _FFLayer(c)])


CACHE_ROUND = 256  # new_cache rounds both capacities up to a multiple of this


class T5Seq2Seq(nn.Module):
    """T5 v1.1 / Flan-T5 encoder-decoder (transformers ``T5ForConditionalGeneration``
    parameter names: ``shared``, ``encoder.*``, ``decoder.*``, ``lm_head``), for
    BLIP-2's Flan-T5 language models.  The encoder takes input EMBEDDINGS (BLIP-2
    puts the projected image queries ahead of the prompt).  ``decode_logits``
    re-runs the decoder over its (short) prefix with the causal relative-position
    bias and cross-attention over the encoder output; ``new_cache`` /
    ``begin_decode`` / ``decode_step`` are the KV-cached form of the same step."""

    def __init__(self, c: T5Config, dec_layers: int | None = None, tie_embeddings: bool = False):
        super().__init__()
        self.cfg = c
        self.tie = tie_embeddings
        self.shared = nn.Embedding(c.vocab, c.d_model)
        self.encoder = nn.Module()
        self.encoder.block = nn.ModuleList([_Block(c, i == 0) for i in range(c.layers)])
        self.encoder.final_layer_norm = T5RMSNorm(c.d_model, c.eps)
        self.decoder = nn.Module()
        self.decoder.block = nn.ModuleList([_DecBlock(c, i == 0) for i in range(dec_layers or c.layers)])
        self.decoder.final_layer_norm = T5RMSNorm(c.d_model, c.eps)
        self.lm_head = Linear(c.d_model, c.vocab, bias=False)
        self.checkpoint_ignore = ("encoder.embed_tokens.", "decoder.embed_tokens.")
        self.cache = None

    @torch.no_grad()
    def encode(self, x: torch.Tensor, mask: torch.Tensor | None = None) -> torch.Tensor:
        bias = self.encoder.block[0].layer[0].SelfAttention.position_bias(x.shape[1], x.device)
        lens = None
        if _fused(x):
            bias, lens = bias.contiguous(), key_lens(mask)
        for blk in self.encoder.block:
            x = blk.layer[0](x, bias, mask, lens)
            x = blk.layer[1](x)
        return self.encoder.final_layer_norm(x)

    @torch.no_grad()
    def decode_logits(self, enc: torch.Tensor, ids: list[int], enc_mask=None) -> torch.Tensor:
        """Next-token logits [vocab] after decoder ids (starting with the
        decoder start token)."""
        dt = self.shared.weight.dtype
        x = self.shared(torch.tensor([ids], device=enc.device)).to(dt)
        s = x.shape[1]
        bias = self.decoder.block[0].layer[0].SelfAttention.position_bias(s, x.device, bidirectional=False)
        bias = bias.masked_fill(torch.ones(s, s, dtype=torch.bool, device=x.device).triu(1)[None], float("-inf"))
        enc_lens = None
        if _fused(x):  # the causal mask stays as -inf entries of the bias
            bias, enc_lens = bias.contiguous(), key_lens(enc_mask)
        for blk in self.decoder.block:
            x = blk.layer[0](x, bias)
            x = blk.layer[1](x, enc, enc_mask, enc_lens)
            x = blk.layer[2](x)
        h = self.decoder.final_layer_norm(x[:, -1:])
        if self.tie:  # tied head (original T5): transformers rescales by d_model^-0.5
            h = (h.float() * self.cfg.d_model ** -0.5).to(h.dtype)
        return self.lm_head(h).float()[0, -1]


    # ---- KV-cached decode ----------------------------------------------------
    def new_cache(self, dec_capacity: int, enc_capacity: int):
        """(Re)use the persistent buffers of the cached decode: per decoder
        layer a self-attention K/V pair [1, cap, H, d_kv] and a cross-attention
        buffer [1, enc_cap, 2, H, d_kv] (K at index 0, V at 1), and the fp32
        [H, cap] table of the self-attention bias by distance (entry d: the
        bias of the key d positions behind the query).  Capacities are rounded
        up to multiples of ``CACHE_ROUND``; buffers that are large enough are
        kept (a captured decode graph stays valid across generations), a
        reallocation drops the graph."""
        c, p = self.cfg, self.lm_head.weight
        kv, xkv = getattr(self, "_kv", None), getattr(self, "_xkv", None)
        if (kv is None or kv[0][0].shape[1] < dec_capacity or xkv[0].shape[1] < enc_capacity
                or kv[0][0].device != p.device or kv[0][0].dtype != p.dtype):
            cap, ecap = (-(-max(int(n), 1) // CACHE_ROUND) * CACHE_ROUND for n in (dec_capacity, enc_capacity))
            if kv is not None and kv[0][0].device == p.device:  # never shrink either buffer
                cap, ecap = max(cap, kv[0][0].shape[1]), max(ecap, xkv[0].shape[1])
            n = len(self.decoder.block)
            z = lambda *shape: torch.zeros(shape, device=p.device, dtype=p.dtype)  # noqa: E731
            self._kv = [(z(1, cap, c.heads, c.d_kv), z(1, cap, c.heads, c.d_kv)) for _ in range(n)]
            self._xkv = [z(1, ecap, 2, c.heads, c.d_kv) for _ in range(n)]
            self._enc_len = torch.zeros(1, dtype=torch.int32, device=p.device)
            self._bias_tab = torch.zeros(c.heads, cap, dtype=torch.float32, device=p.device)
            self._bias_key = None
            self._graph = None
        self.cache = self._kv
        self._ensure_bias_table()

    def _ensure_bias_table(self):
        """Fill the distance table from decoder block 0's relative_attention_bias
        (in place: a captured graph reads this tensor) when it is new or the
        embedding moved or was written."""
        w = self.decoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        key = (w.data_ptr(), w.device, w.dtype, w._version)
        if self._bias_key != key:
            c = self.cfg
            d = torch.arange(self._bias_tab.shape[1], device=self._bias_tab.device)
            bucket = relative_position_bucket(-d, c.buckets, c.max_distance, bidirectional=False)
            self._bias_tab.copy_(w.detach().to(self._bias_tab.device)[bucket].float().t())
            self._bias_key = key

    @property
    def cache_capacity(self) -> int:
        return 0 if self.cache is None else self.cache[0][0].shape[1]

    @torch.no_grad()
    def begin_decode(self, enc: torch.Tensor, enc_mask: torch.Tensor | None = None):
        """Start a generation over encoder states ``enc`` [1, T, d_model]: one
        GEMM per decoder layer against its fused [k; v] cross-attention weight
        fills the cross buffers, and the device-side encoder length is set to
        T, or to the number of set entries of the PREFIX mask ``enc_mask``
        [1, T] (``key_lens``).  The self-attention cache restarts at position 0
        (``decode_step(start_token, 0)``)."""
        t = enc.shape[1]
        if (self.cache is None or self._xkv[0].shape[1] < t or self._xkv[0].device != enc.device
                or self._xkv[0].dtype != self.lm_head.weight.dtype):
            self.new_cache(max(self.cache_capacity, 1), t)
        c = self.cfg
        for blk, xkv in zip(self.decoder.block, self._xkv):
            w, rebuilt = blk.layer[1].EncDecAttention.fuse(("k", "v"))
            xkv[:, :t].copy_(ops.gemm(enc, w, None).view(1, t, 2, c.heads, c.d_kv))
        if enc_mask is None:
            self._enc_len.fill_(t)
        else:
            self._enc_len.copy_(key_lens(enc_mask))

    @torch.no_grad()
    def _decode_fn(self, ids, pos_t, len_t):
        c = self.cfg
        inner = c.heads * c.d_kv
        x = self.shared(ids).to(self.lm_head.weight.dtype)  # [1, 1, d_model]
        for blk, kv, xkv in zip(self.decoder.block, self.cache, self._xkv):
            sa, ca, ff = blk.layer
            a, e, d = sa.SelfAttention, ca.EncDecAttention, ff.DenseReluDense
            qkv = ops.gemv(x, a.fuse(("q", "k", "v"))[0], rms=(sa.layer_norm.weight, sa.layer_norm.eps))
            qkv = qkv.view(1, 1, 3, c.heads, c.d_kv)
            o = ops.decode_attention(qkv[:, :, 0], kv[0], kv[1], 1.0, len_t, k_new=qkv[:, :, 1], v_new=qkv[:, :, 2],
                                     pos=pos_t, rel_bias=self._bias_tab)  # T5: no 1/sqrt(d) scaling
            x = ops.gemv(o.reshape(1, 1, inner), a.o.weight, residual=x)
            q = ops.gemv(x, e.q.weight, rms=(ca.layer_norm.weight, ca.layer_norm.eps)).view(1, 1, c.heads, c.d_kv)
            o = ops.decode_attention(q, xkv[:, :, 0], xkv[:, :, 1], 1.0, self._enc_len)
            x = ops.gemv(o.reshape(1, 1, inner), e.o.weight, residual=x)
            h = ops.gemv_glu(x, d.wi_0.weight, d.wi_1.weight, act="gelu_tanh",
                             rms=(ff.layer_norm.weight, ff.layer_norm.eps))
            x = ops.gemv(h, d.wo.weight, residual=x)
        nf = self.decoder.final_layer_norm
        logits = ops.gemv(x[:, -1], self.lm_head.weight, rms=(nf.weight, nf.eps)).float()[0]
        return logits * c.d_model ** -0.5 if self.tie else logits  # tied head: see decode_logits

    @torch.no_grad()
    def decode_step(self, token: int, pos: int) -> torch.Tensor:
        """Next-token logits [vocab] after appending decoder ``token`` at position
        ``pos`` (the start token at 0) of the self-attention cache, over the
        encoder states of the last ``begin_decode``.  On the GPU the whole step
        replays from one hipGraph; the returned tensor is then overwritten by
        the next step."""
        if self.cache is None or not 0 <= int(pos) < self.cache_capacity:
            raise ValueError(f"T5Seq2Seq.decode_step: position {pos} outside the cache (capacity "
                             f"{self.cache_capacity}): call new_cache / begin_decode first")
        dev = self.lm_head.weight.device
        if any([blk.layer[0].SelfAttention.fuse(("q", "k", "v"))[1] for blk in self.decoder.block]):
            self._graph = None
        self._ensure_bias_table()
        st = getattr(self, "_dstate", None)
        if st is None or st[0].device != dev:
            st = (torch.zeros(1, 1, dtype=torch.long, device=dev), torch.zeros(1, dtype=torch.long, device=dev),
                  torch.zeros(1, dtype=torch.int32, device=dev))
            self._dstate = st
            self._graph = None
        ids, pos_t, len_t = st
        ids.fill_(int(token))
        pos_t.fill_(int(pos))
        len_t.fill_(int(pos) + 1)
        from ..pipelines.graphs import CapturedCall, graphs_enabled

        if not graphs_enabled(dev):
            return self._decode_fn(ids, pos_t, len_t)
        g = getattr(self, "_graph", None)
        if g is None:
            g = CapturedCall(self._decode_fn, ids=ids, pos_t=pos_t, len_t=len_t)
            self._graph = g
        return g.run(ids=ids, pos_t=pos_t, len_t=len_t)


class T5Tokenizer:
    """SentencePiece (``spiece.model``) when present; deterministic hash
    fallback otherwise.  Appends ``</s>`` (id 1), pads with 0 to max_length."""

    def __init__(self, model_dir: str | None = None, max_length: int = 77, vocab: int = 32128, lower: bool = True):
        self.max_length, self.vocab, self.lower = max_length, vocab, lower
        self.sp = None
        path = os.path.join(model_dir, "spiece.model") if model_dir else None
        if path and os.path.exists(path):
            import sentencepiece

            self.sp = sentencepiece.SentencePieceProcessor(model_file=path)

    def encode(self, text: str) -> list[int]:
        # IFPipeline without bs4/ftfy caption cleaning: lower-case + strip
        # (lower=False: the plain tokenizer, e.g. BLIP-2's Flan-T5 prompts)
        text = (text.lower() if self.lower else text).strip()
        if self.sp is not None:
            return list(self.sp.encode(text))
        return [int.from_bytes(hashlib.blake2b(w.encode(), digest_size=8).digest(), "little") % (self.vocab - 100) + 3
                for w in text.split()]

    def decode(self, ids: list[int]) -> str:
        """Text of ``ids`` without pad / eos (``skip_special_tokens``)."""
        ids = [int(i) for i in ids if int(i) not in (0, 1)]
        if self.sp is not None:
            return self.sp.decode(ids)
        return " ".join(f"w{i}" for i in ids)

    def __call__(self, texts: list[str]):
        ids, masks = [], []
        for t in texts:
            x = self.encode(t)[: self.max_length - 1] + [1]
            masks.append([1] * len(x) + [0] * (self.max_length - len(x)))
            ids.append(x + [0] * (self.max_length - len(x)))
        return torch.tensor(ids), torch.tensor(masks, dtype=torch.bool)
