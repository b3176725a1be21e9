"""LLaMA / Vicuna decoder (transformers ``LlamaForCausalLM`` parameter names:
``model.embed_tokens``, ``model.layers.{i}.self_attn.{q,k,v,o}_proj``,
``mlp.{gate,up,down}_proj``, ``input_layernorm`` / ``post_attention_layernorm``,
``model.norm``, ``lm_head``) for InstructBLIP's Vicuna language models.

Pre-RMSNorm blocks; rotary position embedding (rotate-half form, default
theta 10000) on q / k; grouped K/V heads expanded to the query heads; SwiGLU
MLP (SiLU of gate_proj fused into its GEMM epilogue, the residual adds fused
into o_proj / down_proj).  Input embeddings may be given directly (the image
query embeddings precede the prompt).

Greedy decode is KV-cached: ``prefill`` runs the GEMM path above over the whole
prompt once and leaves the post-RoPE keys and the values in per-layer caches;
``decode_step`` then runs one token through the decode kernels, five launches a
layer on the HIP path (``ops.gemv`` of the fused QKV weight with the input
RMSNorm in its prologue; ``ops.decode_attention`` with RoPE, the cache append
and the grouped heads; the o_proj GEMV with the residual; ``ops.gemv_glu`` with
the post-attention RMSNorm; the down_proj GEMV with the residual), the final
norm in the lm_head GEMV's prologue, and the whole step replays from one
hipGraph.  On the CPU the same ops run their torch definitions.
``last_logits`` re-runs a whole sequence without a cache (the A/B of
tools/llamadecodebench.py and the ``use_cache=False`` / ``CSK_DECODE=0`` path of
``Blip2.generate``).
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn as nn

from .. import ops
from .layers import Linear, Prepared


@dataclasses.dataclass
class LlamaConfig:
    vocab: int = 32000
    dim: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 32
    ffn: int = 11008
    eps: float = 1e-6
    theta: float = 10000.0
    bos_id: int = 1
    eos_id: int = 2

    @classmethod
    def from_hf(cls, t: dict) -> "LlamaConfig":
        rope = t.get("rope_parameters") or t.get("rope_scaling") or {}
        if rope.get("rope_type", rope.get("type", "default")) not in ("default", None):
            raise ValueError(f"img2txt: LLaMA rope type {rope.get('rope_type')!r} is not supported")
        return cls(vocab=t.get("vocab_size", 32000), dim=t.get("hidden_size", 4096),
                   layers=t.get("num_hidden_layers", 32), heads=t.get("num_attention_heads", 32),
                   kv_heads=t.get("num_key_value_heads") or t.get("num_attention_heads", 32),
                   ffn=t.get("intermediate_size", 11008), eps=t.get("rms_norm_eps", 1e-6),
                   theta=rope.get("rope_theta", t.get("rope_theta", 10000.0)), bos_id=t.get("bos_token_id", 1),
                   eos_id=t.get("eos_token_id", 2))


class RMSNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.eps = eps

    def forward(self, x):
        xf = x.float()
        return (self.weight.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps))).to(x.dtype)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


class _Attn(Prepared):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.c, self.hd = c, c.dim // c.heads
        self.q_proj = Linear(c.dim, c.heads * self.hd, bias=False)
        self.k_proj = Linear(c.dim, c.kv_heads * self.hd, bias=False)
        self.v_proj = Linear(c.dim, c.kv_heads * self.hd, bias=False)
        self.o_proj = Linear(c.heads * self.hd, c.dim, bias=False)

    def prepare(self):
        """One [(H + 2 Hkv) hd, dim] QKV weight for the decode step's GEMV; the
        three projection weights become row-range views of it (row stride
        ``dim``, so ``Linear`` / ``gemm`` run on them unchanged and no QKV weight
        is resident twice).  State-dict names do not change."""
        projs = (self.q_proj, self.k_proj, self.v_proj)
        w = torch.cat([p.weight.detach() for p in projs], 0)
        r = 0
        for p in projs:
            n = p.weight.shape[0]
            p.weight.data = w[r:r + n]
            r += n
        self.w_qkv = w

    def _ensure(self) -> bool:
        """(Re)build the fused weight if the parameters moved (device, dtype or
        storage: ``.to()``, an assigning load); True if it was rebuilt."""
        w, q = getattr(self, "w_qkv", None), self.q_proj.weight
        if (w is None or w.device != q.device or w.dtype != q.dtype
                or any(p.weight.untyped_storage().data_ptr() != w.untyped_storage().data_ptr()
                       for p in (self.q_proj, self.k_proj, self.v_proj))):
            self.prepare()
            return True
        return False

    def decode(self, x, norm, cache, rope, pos_t, len_t):
        """One-token step with device-side position / length (graph-capturable):
        ``norm`` (the layer's input RMSNorm) runs in the QKV GEMV's prologue; the
        attention kernel rotates q / k, appends k / v and reads the grouped heads."""
        c, hd = self.c, self.hd
        nq, nkv = c.heads * hd, c.kv_heads * hd
        qkv = ops.gemv(x, self.w_qkv, rms=(norm.weight, norm.eps))
        q = qkv[..., :nq].view(1, 1, c.heads, hd)
        k = qkv[..., nq:nq + nkv].view(1, 1, c.kv_heads, hd)
        v = qkv[..., nq + nkv:].view(1, 1, c.kv_heads, hd)
        o = ops.decode_attention(q, cache[0], cache[1], hd ** -0.5, len_t, k_new=k, v_new=v, pos=pos_t, rope=rope)
        return ops.gemv(o.reshape(1, 1, nq), self.o_proj.weight, residual=x)

    def forward(self, h, x, cos, sin, cache=None):
        b, s, _ = h.shape
        q = self.q_proj(h).view(b, s, self.c.heads, self.hd)
        k = self.k_proj(h).view(b, s, self.c.kv_heads, self.hd)
        v = self.v_proj(h).view(b, s, self.c.kv_heads, self.hd)
        qf, kf = q.float(), k.float()
        q = (qf * cos + _rotate_half(qf) * sin).to(h.dtype)
        k = (kf * cos + _rotate_half(kf) * sin).to(h.dtype)
        if cache is not None:  # prefill: post-RoPE keys and the values of positions [0, s)
            cache[0][:, :s].copy_(k)
            cache[1][:, :s].copy_(v)
        if self.c.kv_heads != self.c.heads:
            rep = self.c.heads // self.c.kv_heads
            k, v = k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)
        o = ops.attention(q.contiguous(), k.contiguous(), v.contiguous(), self.hd ** -0.5, causal=True)
        return self.o_proj(o.reshape(b, s, -1), residual=x)


class _MLP(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.gate_proj = Linear(c.dim, c.ffn, bias=False)
        self.up_proj = Linear(c.dim, c.ffn, bias=False)
        self.down_proj = Linear(c.ffn, c.dim, bias=False)

    def forward(self, h, x):
        return self.down_proj(self.gate_proj(h, act="silu") * self.up_proj(h), residual=x)


class _Layer(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.self_attn = _Attn(c)
        self.mlp = _MLP(c)
        self.input_layernorm = RMSNorm(c.dim, c.eps)
        self.post_attention_layernorm = RMSNorm(c.dim, c.eps)


CACHE_ROUND = 256  # new_cache rounds the capacity up to a multiple of this


class LlamaLM(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.cfg = c
        self.cache = None
        self.model = nn.Module()
        self.model.embed_tokens = nn.Embedding(c.vocab, c.dim)
        self.model.layers = nn.ModuleList([_Layer(c) for _ in range(c.layers)])
        self.model.norm = RMSNorm(c.dim, c.eps)
        self.lm_head = Linear(c.dim, c.vocab, bias=False)

    def _rope(self, s, device):
        hd = self.cfg.dim // self.cfg.heads
        inv = 1.0 / (self.cfg.theta ** (torch.arange(0, hd, 2, dtype=torch.float32, device=device) / hd))
        f = torch.arange(s, dtype=torch.float32, device=device)[:, None] * inv[None]
        emb = torch.cat((f, f), -1)
        return emb.cos()[None, :, None], emb.sin()[None, :, None]  # [1, S, 1, hd]

    @torch.no_grad()
    def last_logits(self, x: torch.Tensor) -> torch.Tensor:
        """Next-token logits [vocab] after input embeddings x [1, S, dim]."""
        cos, sin = self._rope(x.shape[1], x.device)
        for lyr in self.model.layers:
            x = lyr.self_attn(lyr.input_layernorm(x), x, cos, sin)
            x = lyr.mlp(lyr.post_attention_layernorm(x), x)
        return self.lm_head(self.model.norm(x[:, -1:])).float()[0, -1]

    # ---- KV-cached decode ----------------------------------------------------
    def new_cache(self, capacity: int):
        """(Re)use the persistent per-layer [1, cap, Hkv, hd] K/V buffers and the
        fp32 RoPE tables [cap, hd / 2] (the formula of ``_rope``).  ``cap`` is
        ``capacity`` rounded up to a multiple of ``CACHE_ROUND``, so growing is
        rare; buffers that are large enough are kept (a captured decode graph
        stays valid across generations), a reallocation drops the graph."""
        c = self.cfg
        p = self.lm_head.weight
        hd = c.dim // c.heads
        kv = getattr(self, "_kv", None)
        if kv is None or kv[0][0].shape[1] < capacity or kv[0][0].device != p.device or kv[0][0].dtype != p.dtype:
            cap = -(-max(int(capacity), 1) // CACHE_ROUND) * CACHE_ROUND
            shape = (1, cap, c.kv_heads, hd)
            self._kv = [(torch.zeros(shape, device=p.device, dtype=p.dtype),
                         torch.zeros(shape, device=p.device, dtype=p.dtype)) for _ in range(c.layers)]
            inv = 1.0 / (c.theta ** (torch.arange(0, hd, 2, dtype=torch.float32, device=p.device) / hd))
            f = torch.arange(cap, dtype=torch.float32, device=p.device)[:, None] * inv[None]
            self._rope_tab = (f.cos().contiguous(), f.sin().contiguous())
            self._graph = None
        self.cache = self._kv

    @property
    def cache_capacity(self) -> int:
        return 0 if self.cache is None else self.cache[0][0].shape[1]

    @torch.no_grad()
    def prefill(self, x: torch.Tensor) -> torch.Tensor:
        """``last_logits`` of input embeddings x [1, S, dim] that also leaves the
        post-RoPE keys and the values of positions [0, S) in the cache (grown
        if it is missing or smaller than S)."""
        s = x.shape[1]
        if self.cache is None or self.cache_capacity < s or self.cache[0][0].device != x.device:
            self.new_cache(s)
        cos, sin = self._rope(s, x.device)
        for lyr, kv in zip(self.model.layers, self.cache):
            x = lyr.self_attn(lyr.input_layernorm(x), x, cos, sin, cache=kv)
            x = lyr.mlp(lyr.post_attention_layernorm(x), x)
        return self.lm_head(self.model.norm(x[:, -1:])).float()[0, -1]

    @torch.no_grad()
    def _decode_fn(self, ids, pos_t, len_t):
        x = self.model.embed_tokens(ids).to(self.lm_head.weight.dtype)  # [1, 1, dim]
        for lyr, kv in zip(self.model.layers, self.cache):
            x = lyr.self_attn.decode(x, lyr.input_layernorm, kv, self._rope_tab, pos_t, len_t)
            n2, mlp = lyr.post_attention_layernorm, lyr.mlp
            h = ops.gemv_glu(x, mlp.gate_proj.weight, mlp.up_proj.weight, act="silu", rms=(n2.weight, n2.eps))
            x = ops.gemv(h, mlp.down_proj.weight, residual=x)
        nf = self.model.norm
        return ops.gemv(x[:, -1], self.lm_head.weight, rms=(nf.weight, nf.eps)).float()[0]

    @torch.no_grad()
    def decode_step(self, token: int, pos: int) -> torch.Tensor:
        """Next-token logits [vocab] after appending ``token`` at position ``pos``
        of the KV cache (positions [0, pos) filled by ``prefill`` / earlier
        steps).  On the GPU the whole step (every layer) replays from one
        hipGraph; the returned tensor is then overwritten by the next step."""
        if self.cache is None or not 0 <= int(pos) < self.cache_capacity:
            raise ValueError(f"LlamaLM.decode_step: position {pos} outside the cache (capacity "
                             f"{self.cache_capacity}): call new_cache / prefill first")
        dev = self.lm_head.weight.device
        if any([lyr.self_attn._ensure() for lyr in self.model.layers]):
            self._graph = None
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
