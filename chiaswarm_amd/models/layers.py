"""Building blocks shared by every model family (UNet, VAE, ControlNet, CLIP,
RRDBNet ...).  Parameter names follow the diffusers / transformers state-dict
key layout so real safetensors checkpoints load unchanged (SURVEY.md §7.1
"state_dict keys compatible with diffusers/HF safetensors"); the compute path
uses *packed* copies made once by ``prepare()`` (NHWC conv weights, fused QKV,
interleaved GEGLU, batched time-embedding projections).

Reference behaviour these mirror: the diffusers pipelines invoked at
swarm/diffusion/diffusion_func.py:96 (UNet / VAE / text encoder forward).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class Prepared(nn.Module):
    """Mixin: ``prepare()`` builds packed inference buffers from parameters."""

    def prepare(self):  # pragma: no cover - overridden
        pass


def prepare_model(model: nn.Module) -> nn.Module:
    """Build packed buffers for every sub-module (call after loading weights)."""
    for m in model.modules():
        if isinstance(m, Prepared):
            m.prepare()
    if hasattr(model, "prepare_self"):
        model.prepare_self()
    return model


class Linear(nn.Linear, Prepared):
    """nn.Linear whose forward runs the MFMA GEMM (fused bias/act/residual)."""

    def forward(self, x, residual=None, act=None, row_stats=False):  # type: ignore[override]
        return ops.gemm(x, self.weight, self.bias, residual=residual, act=act, row_stats=row_stats)


class Conv2d(nn.Conv2d, Prepared):
    """NHWC conv.  ``weight`` keeps the PyTorch [Cout, Cin, kh, kw] layout for
    state-dict compatibility; ``wp`` is the packed [Cout, kh, kw, Cin] copy the
    implicit-GEMM kernel reads."""

    def prepare(self):
        self.wp = ops.pack_conv_weight(self.weight.detach())

    def _wp(self):
        wp = getattr(self, "wp", None)
        if wp is None or wp.device != self.weight.device or wp.dtype != self.weight.dtype:
            self.prepare()
        return self.wp

    def forward(self, x, residual=None, up2x=False, bias2d=None, padding=None, act=None, out_scale=1.0,
                out=None, gn_stats=False, row_stats=False, residual2=None, res_scale=1.0,
                norm=None, norm_optional=False):  # type: ignore[override]
        """``norm``: ``GroupNorm.after_conv(...)`` of the GroupNorm that consumes
        the output (``ops.conv2d``): returns the normalised tensor, or
        (normalised, raw) when the raw output is kept."""
        kh, kw = self.kernel_size
        if (kh == 1 and kw == 1 and self.stride == (1, 1) and not up2x and act is None and out_scale == 1.0
                and out is None and x.is_contiguous() and residual2 is None and res_scale == 1.0 and norm is None):
            w2 = self.weight.view(self.out_channels, self.in_channels)
            gr = x.shape[1] * x.shape[2] if (gn_stats and bias2d is None and x.dim() == 4) else 0
            y = ops.gemm(x, w2, self.bias, residual=residual, gn_rows=gr, row_stats=row_stats and bias2d is None)
            if bias2d is not None:
                y = y + bias2d[:, None, None, :].to(y.dtype)
            return y
        if padding is None:
            ph, pw = self.padding
            pad = ph if ph == pw else (ph, pw, ph, pw)
        else:
            pad = padding
        return ops.conv2d(x, self._wp(), self.bias, self.stride[0], pad, residual=residual,
                          up2x=up2x, bias2d=bias2d, act=act, out_scale=out_scale, out=out,
                          dilation=max(self.dilation), gn_stats=gn_stats, residual2=residual2, res_scale=res_scale,
                          norm=norm, norm_optional=norm_optional)


class Conv1d(nn.Conv1d, Prepared):
    """1-D conv on token-layout [B, T, C] tensors (state dict = nn.Conv1d);
    runs the implicit-GEMM conv kernel on the [B, 1, T, C] view with a (1, k)
    packed kernel.  Only stride 1 (HiFi-GAN / EnCodec decoder convs)."""

    def prepare(self):
        self.wp = self.weight.detach().permute(0, 2, 1).unsqueeze(1).contiguous()  # [Cout, 1, k, Cin]

    def _wp(self):
        wp = getattr(self, "wp", None)
        if wp is None or wp.device != self.weight.device or wp.dtype != self.weight.dtype:
            self.prepare()
        return self.wp

    def forward(self, x, act=None, residual=None, out_scale=1.0, out=None, padding=None):  # type: ignore[override]
        assert self.stride == (1,), "Conv1d: stride 1 only"
        p = self.padding[0] if padding is None else padding
        return ops.conv1d(x, self._wp(), self.bias, padding=p, dilation=self.dilation[0], act=act,
                          residual=residual, out_scale=out_scale, out=out)


class ConvTranspose1d(nn.ConvTranspose1d, Prepared):
    """Transposed 1-D conv on [B, T, C] as ``stride`` polyphase convolutions
    (``ops.pack_conv_transpose1d``): no zero-insertion."""

    def prepare(self):
        self.phases = ops.pack_conv_transpose1d(self.weight.detach(), self.stride[0], self.padding[0])

    def forward(self, x, act=None):  # type: ignore[override]
        ph = getattr(self, "phases", None)
        if ph is None or (ph[0][0] is not None and (ph[0][0].device != self.weight.device
                                                    or ph[0][0].dtype != self.weight.dtype)):
            self.prepare()
        return ops.conv_transpose1d(x, self.weight, self.bias, self.stride[0], self.padding[0], self.phases, act)


class GroupNorm(nn.GroupNorm):
    def forward(self, x, silu=False):  # type: ignore[override]
        pre = getattr(x, "_csk_prenorm", None)
        if pre is not None and pre[0] == self._key(silu):
            return pre[1]  # the producer conv already applied this norm (ResnetBlock2D next_norm)
        return ops.group_norm(x, self.weight, self.bias, self.num_groups, self.eps, silu=silu)

    def _key(self, silu):
        w, b = self.weight, self.bias
        return (w.data_ptr(), w._version, b.data_ptr(), b._version, self.num_groups, self.eps, bool(silu))

    def attach(self, raw, normed, silu=False):
        """Carry ``normed`` = this norm of ``raw`` on ``raw`` (as ``_csk_gn`` carries
        statistics): ``forward(raw)`` returns it; any other consumer ignores it.
        As with ``_csk_gn``, ``raw`` must not be modified in place while it carries
        the attribute: the key covers this norm's parameters, not ``raw``'s values."""
        if normed is not None:
            raw._csk_prenorm = (self._key(silu), normed)
        return raw

    def after_conv(self, silu=False, keep_raw=False):
        """This norm as the ``norm`` argument of the conv that produces its input."""
        return (self.weight, self.bias, self.num_groups, self.eps, silu, keep_raw)


class LayerNorm(nn.LayerNorm):
    def forward(self, x):  # type: ignore[override]
        return ops.layer_norm(x, self.weight, self.bias, self.eps)


# ----------------------------------------------------------------------------
# Attention (self / cross), diffusers naming: to_q / to_k / to_v / to_out.0
# ----------------------------------------------------------------------------
class Attention(Prepared):
    def __init__(self, query_dim, heads, dim_head, cross_dim=None, bias=False, out_bias=True,
                 norm_groups=None, norm_eps=1e-6, residual=False):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head = heads, dim_head
        self.is_cross = cross_dim is not None
        kv_dim = cross_dim if cross_dim is not None else query_dim
        self.to_q = Linear(query_dim, inner, bias=bias)
        self.to_k = Linear(kv_dim, inner, bias=bias)
        self.to_v = Linear(kv_dim, inner, bias=bias)
        self.to_out = nn.ModuleList([Linear(inner, query_dim, bias=out_bias)])
        self.group_norm = GroupNorm(norm_groups, query_dim, eps=norm_eps) if norm_groups else None
        self.residual = residual
        self.scale = 1.0 / math.sqrt(dim_head)

    def prepare(self):
        q, k, v = self.to_q, self.to_k, self.to_v
        if self.is_cross:
            self.w_kv = torch.cat([k.weight, v.weight], 0).detach()
            self.b_kv = torch.cat([k.bias, v.bias], 0).detach() if k.bias is not None else None
        else:
            self.w_qkv = torch.cat([q.weight, k.weight, v.weight], 0).detach()
            self.b_qkv = (torch.cat([q.bias, k.bias, v.bias], 0).detach()
                          if q.bias is not None else None)

    def _ensure(self):
        attr = "w_kv" if self.is_cross else "w_qkv"
        w = getattr(self, attr, None)
        if w is None or w.device != self.to_q.weight.device or w.dtype != self.to_q.weight.dtype:
            self.prepare()

    def context_kv(self, ctx):
        """K/V of a cross-attention for a fixed context: [B, Skv, 2, H, D].
        Constant over all denoising steps -> computed once per request."""
        self._ensure()
        b, s, _ = ctx.shape
        kv = ops.gemm(ctx, self.w_kv, self.b_kv)
        return kv.view(b, s, 2, self.heads, self.dim_head)

    def forward(self, x, ctx=None, kv=None, residual=None, causal=False):
        """x: [B, S, C].  ``residual`` is added in the out-projection epilogue."""
        self._ensure()
        if self.is_cross:
            return self.attend_q(self.to_q(x), kv, ctx if ctx is not None else x, residual)
        return self.attend_qkv(ops.gemm(x, self.w_qkv, self.b_qkv), residual, causal=causal)

    def attend_qkv(self, qkv, residual=None, causal=False, row_stats=False, project=True):
        """Self-attention from the fused QKV projection [B, S, 3*H*D].
        ``project=False``: the attention output [B, S, H*D] itself, for a
        consumer that runs the out-projection (the fused cross-attention block)."""
        b, s, _ = qkv.shape
        h, d = self.heads, self.dim_head
        qkv = qkv.view(b, s, 3, h, d)
        store = self.__dict__.get("_store_probs")
        if store is not None:  # SAG (pipelines/guided.py): the softmax(q k^T) map of this layer, fp32
            q, k = qkv[:, :, 0].float().transpose(1, 2), qkv[:, :, 1].float().transpose(1, 2)
            store.append(torch.softmax(q @ k.transpose(-1, -2) * self.scale, dim=-1))
        o = ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], self.scale, causal=causal)
        if not project:
            return o.reshape(b, s, h * d)
        return self.to_out[0](o.reshape(b, s, h * d), residual=residual, row_stats=row_stats)

    def attend_q(self, q, kv, ctx, residual=None, row_stats=False):
        """Cross-attention from the query projection [B, S, H*D]; ``kv`` per-request
        K/V ([B, Skv, 2, H, D]) or None (computed from ``ctx``)."""
        b, s, _ = q.shape
        h, d = self.heads, self.dim_head
        if kv is None:  # no context given: attend to itself (diffusers attn2 semantics)
            kv = self.context_kv(ctx)
        store = self.__dict__.get("_store_probs")
        if store is not None:  # Attend-and-Excite (pipelines/guided.py): softmax(q k^T), fp32, in the autograd graph
            qf, kf = q.view(b, s, h, d).float().transpose(1, 2), kv[:, :, 0].float().transpose(1, 2)
            store.append(torch.softmax(qf @ kf.transpose(-1, -2) * self.scale, dim=-1))
        o = ops.attention(q.view(b, s, h, d), kv[:, :, 0], kv[:, :, 1], self.scale)
        return self.to_out[0](o.reshape(b, s, h * d), residual=residual, row_stats=row_stats)


class SpatialSelfAttention(Attention):
    """Single-head VAE mid-block attention on NHWC maps (GroupNorm + residual)."""

    def __init__(self, channels, norm_groups=32, eps=1e-6):
        super().__init__(channels, 1, channels, bias=True, norm_groups=norm_groups, norm_eps=eps)

    def forward(self, x):  # type: ignore[override]
        b, hh, ww, c = x.shape
        hN = self.group_norm(x).view(b, hh * ww, c)
        out = super().forward(hN, residual=x.view(b, hh * ww, c))
        return out.view(b, hh, ww, c)


class GEGLU(Prepared):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)

    def prepare(self):
        self.wp, self.bp = ops.pack_geglu(self.proj.weight.detach(),
                                          self.proj.bias.detach() if self.proj.bias is not None else None)

    def ensure(self):
        wp = getattr(self, "wp", None)
        if wp is None or wp.device != self.proj.weight.device or wp.dtype != self.proj.weight.dtype:
            self.prepare()

    def forward(self, x):
        self.ensure()
        return ops.gemm(x, self.wp, self.bp, act="geglu")


class FeedForward(Prepared):
    """diffusers FeedForward(GEGLU): keys ff.net.0.proj / ff.net.2."""

    def __init__(self, dim, mult=4):
        super().__init__()
        inner = dim * mult
        self.inner = inner
        self.net = nn.ModuleList([GEGLU(dim, inner), nn.Identity(), Linear(inner, dim)])

    def prepare(self):
        """Packed weights of the fused FF kernel (csrc/kernels/ff.hip), C = 320
        only (the blocks it serves)."""
        p, d = self.net[0].proj, self.net[2]
        if p.weight.shape[1] != 320:
            self.ff_w1p = self.ff_b1p = self.ff_w2p = None
            return
        self.ff_w1p, self.ff_b1p, self.ff_w2p = ops.pack_ff_fused(
            p.weight.detach(), None if p.bias is None else p.bias.detach(), d.weight.detach())

    def fused_weights(self):
        w = getattr(self, "ff_w1p", None)
        p = self.net[0].proj.weight
        if (w is None and p.shape[1] == 320) or (w is not None and (w.device != p.device or w.dtype != p.dtype)):
            self.prepare()
        return getattr(self, "ff_w1p", None), getattr(self, "ff_b1p", None), getattr(self, "ff_w2p", None)

    def forward(self, x, residual=None):
        return self.net[2](self.net[0](x), residual=residual)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, heads, dim_head, cross_dim):
        super().__init__()
        self.norm1 = LayerNorm(dim)
        self.attn1 = Attention(dim, heads, dim_head)
        self.norm2 = LayerNorm(dim)
        self.attn2 = Attention(dim, heads, dim_head, cross_dim=cross_dim)
        self.norm3 = LayerNorm(dim)
        self.ff = FeedForward(dim)

    def _fold(self, name, w, b, norm):
        """gamma/beta-folded copy of a projection that consumes ``norm`` (cached;
        refolded when the weights change, e.g. a LoRA merge)."""
        key = (w.data_ptr(), w._version, norm.weight.data_ptr(), norm.weight._version, w.dtype, w.device)
        folds = self.__dict__.setdefault("_ln_folds", {})
        f = folds.get(name)
        if f is None or f[0] != key:
            f = (key, ops.fold_layer_norm(w.detach(), None if b is None else b.detach(), norm.weight.detach(),
                                          None if norm.bias is None else norm.bias.detach()))
            folds[name] = f
        return f[1]

    def forward(self, x, ctx=None, kv=None, row_stats=None, dup=False, qkv=None, tail=None):
        """``qkv``: this block's self-attention projection LN1(x) Wqkv^T already
        computed (the fused transformer-input kernel, Transformer2D.forward).
        ``tail = (wpp, bp, xin, gn_rows)``: the transformer's proj_out (packed,
        ``ops.pack_ff_proj``), its residual and the rows per sample of the
        GroupNorm statistics; where the fused feed-forward takes it
        (``ops.ff_proj_fusable``) the block returns ``(z, True)``, z = xin +
        proj_out(block output) shaped like ``xin``, else ``(block output, False)``.

        On the HIP path every LayerNorm runs inside the GEMM that consumes it
        (``ops.layer_norm_gemm``): each producer GEMM (proj_in, the attention
        out-projections, the FF down-projection) emits per-row statistics of its
        output, so the three LN kernels per block disappear.  ``row_stats``: emit
        them for whatever consumes this block's output (default: on HIP).
        ``dup``: ``x`` is one CFG half (UNet2DConditionModel.forward cfg_dup):
        self-attention and the cross-attention query run on it, and the query and
        residual are duplicated for the cross-attention (whose context differs
        between the halves)."""
        hip = ops.row_stats_wanted(x)
        if row_stats is None:
            row_stats = hip
        a1, a2, ff = self.attn1, self.attn2, self.ff
        a1._ensure()
        if qkv is None:
            fus = ops.ln_fusable(x)
            qkv = ops.layer_norm_gemm(x, self.norm1, a1.w_qkv, a1.b_qkv,
                                      self._fold("qkv", a1.w_qkv, a1.b_qkv, self.norm1) if fus else None)
        if hip and kv is not None and x.dim() == 3 and ops.xattn_pre_fusable(x, kv, x.shape[1], dup):
            # the fused cross-attention kernel below (csrc/kernels/xattn.hip) with the
            # self-attention out-projection + residual as its prologue: its input never
            # reaches HBM; with ``dup`` one launch serves both CFG halves straight from
            # the half-batch attention output
            f = self._fold("q", a2.to_q.weight, a2.to_q.bias, self.norm2)
            hit = self.__dict__.get("_q_perm")
            if hit is None or hit[0] is not f:
                hit = (f, ops.permute_xattn_q(f[0]))
                self.__dict__["_q_perm"] = hit
            o = a1.attend_qkv(qkv, project=False)
            x = ops.xattn_block(None, hit[1], f[1], f[2], kv, a2.to_out[0].weight, a2.to_out[0].bias, self.norm2.eps,
                                a2.scale, x.shape[1], row_stats=hip,
                                pre=(o, x, a1.to_out[0].weight, a1.to_out[0].bias),
                                batch=(2 if dup else 1) * x.shape[0])
            return self._ff_tail(x, row_stats, hip, tail)
        x = a1.attend_qkv(qkv, residual=x, row_stats=hip)
        if hip and not dup and kv is not None and x.dim() == 3 and ops.xattn_fusable(x, kv, x.shape[1]):
            # LN2 + Q projection + attention over the context + out-projection +
            # residual in ONE kernel (csrc/kernels/xattn.hip)
            w2, colsum, b2 = self._fold("q", a2.to_q.weight, a2.to_q.bias, self.norm2)
            x = ops.xattn_block(x, w2, colsum, b2, kv, a2.to_out[0].weight, a2.to_out[0].bias, self.norm2.eps,
                                a2.scale, x.shape[1], row_stats=hip)
        elif hip and not dup and kv is not None and x.dim() == 3 and ops.qattn_fusable(x, kv, x.shape[1]):
            # LN2 + Q projection with the attention in its epilogue (the query
            # tensor and the short-KV attention launch disappear), then the
            # out-projection + residual
            fus = ops.ln_fusable(x)
            o = ops.layer_norm_gemm_attn(x, self.norm2, a2.to_q.weight, a2.to_q.bias,
                                         self._fold("q", a2.to_q.weight, a2.to_q.bias, self.norm2) if fus else None,
                                         kv, a2.scale, x.shape[1])
            x = a2.to_out[0](o, residual=x, row_stats=hip)
        else:
            fus = ops.ln_fusable(x)
            q = ops.layer_norm_gemm(x, self.norm2, a2.to_q.weight, a2.to_q.bias,
                                    self._fold("q", a2.to_q.weight, a2.to_q.bias, self.norm2) if fus else None)
            if dup:
                q, x = ops.dup2(q), ops.dup2(x)
            x = a2.attend_q(q, kv, ctx if ctx is not None else x, residual=x, row_stats=hip)
        return self._ff_tail(x, row_stats, hip, tail)

    def _ff_tail(self, x, row_stats, hip, tail):
        """The feed-forward sub-block (and ``tail``, see ``forward``)."""
        ff = self.ff
        if hip and not row_stats and ops.ff_fusable(x, ff.inner):
            # LN3 + GEGLU + down-projection + residual in ONE kernel
            # (csrc/kernels/ff.hip): the [M, 4C] intermediate never reaches HBM
            w1p, b1p, w2p = ff.fused_weights()
            seg = ops.ff_proj_fusable(x, ff.inner, tail[3]) if tail is not None and w1p is not None else 0
            if seg:
                # ... and the transformer's proj_out + residual + GroupNorm
                # statistics in the same kernel: the FF output stays on chip too
                wpp, bp, xin, gn_rows = tail
                return ops.ff_fused_proj(x, self.norm3.weight, self.norm3.bias, w1p, b1p, w2p, ff.net[2].bias, wpp, bp,
                                         xin, self.norm3.eps, gn_rows, seg), True
            if w1p is not None:
                y = ops.ff_fused(x, self.norm3.weight, self.norm3.bias, w1p, b1p, w2p, ff.net[2].bias,
                                 self.norm3.eps)
                return y if tail is None else (y, False)
        g = ff.net[0]
        g.ensure()
        fus = ops.ln_fusable(x)
        hdn = ops.layer_norm_gemm(x, self.norm3, g.wp, g.bp, self._fold("ff", g.wp, g.bp, self.norm3) if fus else None,
                                  act="geglu")
        y = ff.net[2](hdn, residual=x, row_stats=row_stats)
        return y if tail is None else (y, False)


class Transformer2D(nn.Module):
    """Spatial transformer: GN -> proj_in -> N x BasicTransformerBlock -> proj_out (+x)."""

    def __init__(self, channels, heads, cross_dim, layers=1, linear_proj=True, groups=32):
        super().__init__()
        dim_head = channels // heads
        self.norm = GroupNorm(groups, channels, eps=1e-6)
        self.linear_proj = linear_proj
        if linear_proj:
            self.proj_in = Linear(channels, channels)
            self.proj_out = Linear(channels, channels)
        else:
            self.proj_in = Conv2d(channels, channels, 1)
            self.proj_out = Conv2d(channels, channels, 1)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(channels, heads, dim_head, cross_dim) for _ in range(layers)])

    def cross_modules(self):
        return [blk.attn2 for blk in self.transformer_blocks]

    def _xin_weights(self):
        """Packed weights of the fused transformer-input kernel (GroupNorm +
        proj_in + block 0's LN1 + QKV, csrc/kernels/xin.hip); refolded when any
        of them changes (e.g. a LoRA merge)."""
        blk = self.transformer_blocks[0]
        a1 = blk.attn1
        a1._ensure()
        wi = self.proj_in.weight
        key = (wi.data_ptr(), wi._version, a1.w_qkv.data_ptr(), a1.w_qkv._version, blk.norm1.weight._version,
               wi.device, wi.dtype)
        hit = self.__dict__.get("_xin")
        if hit is None or hit[0] != key:
            w2, colsum, b2 = blk._fold("qkv", a1.w_qkv, a1.b_qkv, blk.norm1)
            c = wi.shape[0]
            hit = (key, ops.pack_xin_qkv(wi.detach().reshape(c, c), None if self.proj_in.bias is None
                                         else self.proj_in.bias.detach(), w2, colsum, b2))
            self.__dict__["_xin"] = hit
        return hit[1]

    def _proj_tail(self, x):
        """proj_out packed for the tail of the last block's fused feed-forward
        (csrc/kernels/ff.hip, PROJ variant), or None where it cannot ride there:
        a C x C ``Linear`` at C = 320 and a contiguous bf16 residual.  Repacked
        when the weight changes (e.g. a LoRA merge)."""
        po = self.proj_out
        c = x.shape[-1]
        if (not isinstance(po, Linear) or not self.transformer_blocks or c != 320 or tuple(po.weight.shape) != (c, c)
                or x.dtype != torch.bfloat16 or po.weight.dtype != torch.bfloat16 or not x.is_contiguous()
                or not ops.row_stats_wanted(x)):
            return None
        w = po.weight
        key = (w.data_ptr(), w._version, w.device, w.dtype)
        hit = self.__dict__.get("_ffproj")
        if hit is None or hit[0] != key:
            hit = (key, ops.pack_ff_proj(w.detach()))
            self.__dict__["_ffproj"] = hit
        return hit[1]

    def _xin_ok(self, x) -> bool:
        if not ops.row_stats_wanted(x) or not self.transformer_blocks:
            return False
        c = x.shape[-1]
        a1 = self.transformer_blocks[0].attn1
        w = self.proj_in.weight
        return (w.shape[0] == c and w.numel() == c * c and a1.to_q.weight.shape[0] == c and not a1.is_cross
                and ops.xin_fusable(x, self.norm.num_groups))

    def forward(self, x, ctx=None, kvs=None, dup=False):
        """``dup``: ``x`` is one CFG half; the first block's cross-attention
        doubles the batch (BasicTransformerBlock.forward) and the output is the
        full batch.  On the HIP path at C = 320 the GroupNorm, proj_in and block
        0's LayerNorm + QKV projection run as ONE kernel (ops.xin_qkv)."""
        b, hh, ww, c = x.shape
        hip = ops.row_stats_wanted(x)
        qkv0 = None
        got = None
        if self._xin_ok(x):
            got = ops.xin_qkv(x, self.norm.weight, self.norm.bias, self.norm.num_groups, self.norm.eps,
                              self._xin_weights(), self.transformer_blocks[0].norm1.eps)
        if got is not None:
            h, qkv0 = got[0].view(b, hh * ww, c), got[1].view(b, hh * ww, 3 * c)
        else:
            h = self.norm(x)
            h = self.proj_in(h, row_stats=hip)  # row statistics feed block 0's fused LayerNorm
            rows = getattr(h, "_csk_rows", None)
            h = h.view(b, hh * ww, c)
            if rows is not None:
                h._csk_rows = rows
        nb = len(self.transformer_blocks)
        wpp = self._proj_tail(x)  # proj_out rides in the last block's fused feed-forward where it can
        for i, blk in enumerate(self.transformer_blocks):
            d = dup and i == 0
            if d:
                x, b = ops.dup2(x), 2 * b
            tail = (wpp, self.proj_out.bias, x, hh * ww) if wpp is not None and i + 1 == nb else None
            h = blk(h, ctx=ctx, kv=None if kvs is None else kvs[i], row_stats=hip and i + 1 < nb, dup=d,
                    qkv=qkv0 if i == 0 else None, tail=tail)
            if tail is not None:
                h, done = h
                if done:
                    return h
        if isinstance(self.proj_out, Linear):
            return ops.gemm(h.view(b, hh, ww, c), self.proj_out.weight, self.proj_out.bias, residual=x,
                            gn_rows=hh * ww)
        return self.proj_out(h.view(b, hh, ww, c), residual=x, gn_stats=True)


class ResnetBlock2D(Prepared):
    """GroupNorm -> conv1 (+ time embedding) -> GroupNorm -> conv2 (+ shortcut).

    A 1x1 ``conv_shortcut`` (``cin != cout``) is no kernel of its own where
    ``ops.SC_FUSE`` is on and every channel count is a multiple of 64: its input
    (both halves of a skip concat in ``forward_cat``) rides along as extra K
    segments of conv2 (``ops.conv2d(extra=...)``), one fp32 accumulation, from
    ONE packed [Cout, 9 Cout + Cin] weight and the folded bias built by
    ``prepare()``.  The parameters (state-dict keys) are unchanged."""

    def __init__(self, cin, cout, temb_channels=None, groups=32, eps=1e-5, groups_out=None):
        super().__init__()
        self.norm1 = GroupNorm(groups, cin, eps=eps)
        self.conv1 = Conv2d(cin, cout, 3, padding=1)
        self.time_emb_proj = Linear(temb_channels, cout) if temb_channels else None
        self.norm2 = GroupNorm(groups_out or groups, cout, eps=eps)
        self.conv2 = Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = Conv2d(cin, cout, 1, padding=0) if cin != cout else None
        self.out_channels = cout

    def prepare(self):
        """Drop the fused shortcut pack; it is rebuilt from the current weights
        on first use (``_sc_pack``: also after a device / dtype change or an
        in-place weight update, e.g. a LoRA merge)."""
        self.__dict__["_scf"] = None

    def _sc_static(self) -> bool:
        sc, c2 = self.conv_shortcut, self.conv2
        return (sc is not None and sc.kernel_size == (1, 1) and sc.stride == (1, 1) and sc.padding == (0, 0)
                and c2.kernel_size == (3, 3) and c2.stride == (1, 1) and c2.padding == (1, 1)
                and c2.dilation == (1, 1) and sc.in_channels % 64 == 0 and c2.in_channels % 64 == 0
                and c2.out_channels % 64 == 0 and self.norm1.weight.dim() == 1 and self.norm2.weight.dim() == 1)

    def _sc_pack(self):
        """(conv2 weight view [Cout, 3, 3, C], shortcut weight view [Cout, Cin],
        folded bias) of one [Cout, 9 C + Cin] matrix.  While the pack is in use
        conv2's own packed copy is released (``Conv2d._wp`` rebuilds it on demand)."""
        sc, c2 = self.conv_shortcut, self.conv2
        w2, ws, b2, bs = c2.weight, sc.weight, c2.bias, sc.bias
        key = (w2.data_ptr(), w2._version, ws.data_ptr(), ws._version, None if b2 is None else b2._version,
               None if bs is None else bs._version, w2.device, w2.dtype)
        hit = self.__dict__.get("_scf")
        if hit is None or hit[0] != key:
            _, wv, (wsc,) = ops.pack_conv_extra(ops.pack_conv_weight(w2.detach()),
                                                [ws.detach().reshape(sc.out_channels, sc.in_channels)])
            bias = None
            if b2 is not None or bs is not None:  # fp32 sum, rounded once
                bias = sum(b.detach().float() for b in (b2, bs) if b is not None).to(w2.dtype)
            hit = (key, (wv, wsc, bias))
            self.__dict__["_scf"] = hit
        if c2.__dict__.get("wp") is not None:
            c2.wp = None
        return hit[1]

    def _sc_fuse(self, srcs):
        """The shortcut of ``srcs`` (channel concat) as conv2's extra K segments:
        (weight view, ((src, weight view), ...), bias), or None (unfused)."""
        if not ops.SC_FUSE or not self._sc_static():
            return None
        cs = [int(t.shape[-1]) for t in srcs]
        if sum(cs) != self.conv_shortcut.in_channels or any(c % 64 for c in cs) or any(t.dim() != 4 for t in srcs):
            return None
        wv, wsc, bias = self._sc_pack()
        extra, off = [], 0
        for t, c in zip(srcs, cs):
            extra.append((t, wsc[:, off:off + c]))
            off += c
        return wv, tuple(extra), bias

    def _shortcut(self, srcs):
        """The unfused 1x1 shortcut of the channel concat ``srcs``."""
        sc_conv = self.conv_shortcut
        if len(srcs) == 1:
            return sc_conv(srcs[0])
        a, b = srcs
        w = sc_conv.weight.view(sc_conv.out_channels, sc_conv.in_channels)
        ca = a.shape[-1]
        return ops.gemm(b, w[:, ca:], sc_conv.bias, residual=ops.gemm(a, w[:, :ca]))

    def _conv2(self, h, sc, next_norm, fuse=None):
        """conv2 + shortcut; ``next_norm``: the GroupNorm the caller knows to
        consume the block output next (a transformer's input norm).  A split-K
        conv2 then applies it in its reduce kernel beside the raw output and the
        result rides on the output (``GroupNorm.attach``).  ``fuse``
        (``_sc_fuse``): the shortcut runs inside conv2, ``sc`` is its sources."""
        conv2 = lambda residual, **kw: self.conv2(h, residual=residual, **kw)  # noqa: E731
        if fuse is not None:
            wv, extra, bias = fuse
            if ops.conv_extra_fusable(h, wv, extra):
                conv2 = lambda residual, **kw: ops.conv2d(h, wv, bias, 1, 1, extra=extra, **kw)  # noqa: E731
                sc = None
            else:
                sc = self._shortcut(sc)
        if next_norm is None or next_norm.weight.dim() != 1:
            return conv2(sc, gn_stats=True)  # block output usually feeds the next GroupNorm
        yn, out = conv2(sc, norm=next_norm.after_conv(keep_raw=True), norm_optional=True)
        return next_norm.attach(out, yn)

    def forward(self, x, temb_proj=None, next_norm=None):
        """``temb_proj``: this block's [B, Cout] time projection (already
        computed by the model's batched time-embedding GEMM).  An unfused 1x1
        shortcut runs on a side stream, overlapping norm1 / conv1 / norm2."""
        fuse = self._sc_fuse((x,))
        if fuse is not None:
            h = self.norm1(x, silu=True)
            h = self.conv1(h, bias2d=temb_proj, norm=self.norm2.after_conv(silu=True))
            return self._conv2(h, (x,), next_norm, fuse)
        sc = x
        with ops.side_branch(x) as br:
            if self.conv_shortcut is not None:
                sc = self.conv_shortcut(x)
        h = self.norm1(x, silu=True)
        # nobody but norm2 reads conv1's output: a split-K conv1 applies norm2 in its
        # reduce kernel, any other takes norm2's statistics from its epilogue
        h = self.conv1(h, bias2d=temb_proj, norm=self.norm2.after_conv(silu=True))
        br.join()
        return self._conv2(h, sc, next_norm)

    def forward_cat(self, a, b, temb_proj=None, next_norm=None):
        """forward() of the channel concat [a | b] (a UNet skip connection)
        without materialising the concat on the HIP path: norm1 reads both
        tensors in place and the 1x1 shortcut reads them as two K segments of
        conv2 (unfused: two accumulating GEMMs; the concat cost a full read +
        write of both tensors per up-block ResNet)."""
        sc_conv = self.conv_shortcut
        hn = None
        if ops.use_hip(a) and sc_conv is not None and sc_conv.kernel_size == (1, 1) and self.norm1.weight.dim() == 1:
            hn = ops.group_norm_cat(a, b, self.norm1.weight, self.norm1.bias, self.norm1.num_groups,
                                    self.norm1.eps, silu=True)
        if hn is None:
            return self.forward(ops.cat_channels(a, b), temb_proj, next_norm)
        fuse = self._sc_fuse((a, b))
        if fuse is not None:
            h = self.conv1(hn, bias2d=temb_proj, norm=self.norm2.after_conv(silu=True))
            return self._conv2(h, (a, b), next_norm, fuse)
        w = sc_conv.weight.view(sc_conv.out_channels, sc_conv.in_channels)
        ca = a.shape[-1]
        with ops.side_branch(a) as br:  # shortcut GEMMs overlap conv1 / norm2
            sc = ops.gemm(a, w[:, :ca])
            sc = ops.gemm(b, w[:, ca:], sc_conv.bias, residual=sc)
        h = self.conv1(hn, bias2d=temb_proj, norm=self.norm2.after_conv(silu=True))
        br.join()
        return self._conv2(h, sc, next_norm)


class Downsample2D(nn.Module):
    def __init__(self, channels, padding=1):
        super().__init__()
        self.conv = Conv2d(channels, channels, 3, stride=2, padding=padding)
        self.pad_asym = padding == 0  # VAE encoder: F.pad(0,1,0,1) then conv s2 p0

    def forward(self, x):
        if self.pad_asym:
            return self.conv(x, padding=(0, 0, 1, 1), gn_stats=True)
        return self.conv(x, gn_stats=True)


class Upsample2D(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = Conv2d(channels, channels, 3, padding=1)

    def forward(self, x, size=None):
        """Nearest x2 fused into the conv's input addressing; an explicit
        ``size`` that is not exactly 2x (odd skip sizes, e.g. AudioLDM's mel
        latents — diffusers' ``forward_upsample_size``) interpolates first."""
        b, h, w, c = x.shape
        if size is None or (int(size[0]), int(size[1])) == (2 * h, 2 * w):
            return self.conv(x, up2x=True, gn_stats=True)
        xi = F.interpolate(x.permute(0, 3, 1, 2), size=(int(size[0]), int(size[1])), mode="nearest")
        return self.conv(xi.permute(0, 2, 3, 1).contiguous(), gn_stats=True)


def timestep_embedding(t: torch.Tensor, dim: int, flip_sin_to_cos=True, shift=0.0,
                       max_period=10000.0) -> torch.Tensor:
    """Sinusoidal embedding (diffusers ``Timesteps``); fp32 output [B, dim]."""
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(half, dtype=torch.float32, device=t.device)
    exponent = exponent / (half - shift)
    emb = t.float()[:, None] * torch.exp(exponent)[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    if flip_sin_to_cos:
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
    return emb


class TimestepEmbedding(nn.Module):
    def __init__(self, cin, dim):
        super().__init__()
        self.linear_1 = Linear(cin, dim)
        self.linear_2 = Linear(dim, dim)

    def forward(self, x):
        return self.linear_2(self.linear_1(x, act="silu"))


def init_random_(model: nn.Module, seed: int = 0, std_scale: float = 1.0):
    """Deterministic random init (no checkpoints offline): N(0, 1/fan_in)
    weights, zero biases, unit norms.  Keeps activations O(1) through deep
    stacks so random-weight benchmarks do not overflow bf16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() >= 2:
                fan_in = p[0].numel()
                std = std_scale / math.sqrt(fan_in)
                if name.endswith("embedding.weight") or "embedding" in name and p.dim() == 2 and "linear" not in name:
                    std = 0.02
                t = torch.randn(p.shape, generator=g, dtype=torch.float32) * std
                p.copy_(t.to(p.dtype))
            elif name.endswith("bias"):
                p.zero_()
            else:  # norm weights
                p.fill_(1.0)
    return model


def init_random_fast_(model: nn.Module, seed: int = 0, std_scale: float = 1.0):
    """Same distribution as ``init_random_`` but generated on the parameter's
    device (seconds instead of minutes for 2.6B-parameter SDXL on the GPU)."""
    dev = next(model.parameters()).device
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() >= 2:
                fan_in = p[0].numel()
                std = std_scale / math.sqrt(fan_in)
                if "embedding" in name and "linear" not in name:
                    std = 0.02
                p.copy_((torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32) * std).to(p.dtype))
            elif name.endswith("bias"):
                p.zero_()
            else:
                p.fill_(1.0)
    return model
