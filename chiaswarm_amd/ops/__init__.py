"""Op layer: every hot op of the UNet / VAE / text-encoder / RRDB stacks.

Layout conventions (MI355X-first):
  * image activations are NHWC  ``[B, H, W, C]`` (C contiguous) end to end;
  * token activations are ``[B, S, C]``;
  * conv weights are packed ``[Cout, kh, kw, Cin]`` (K-contiguous rows of the
    implicit GEMM), linear weights ``[N, K]``;
  * attention q/k/v are ``[B, S, H, D]`` views (D contiguous; any B/S/H strides),
    so a fused QKV projection output ``[B, S, 3, H, D]`` is consumed in place.

Each op has one plain-PyTorch definition (``_ref_*``), used for CPU tensors and
in ``reference`` mode, and one gfx950 kernel in libcsk.so (``hip_ops``).
"""
from __future__ import annotations

import math

import os

import torch
import torch.nn.functional as F

from . import _lib  # noqa: F401
from .mode import get_mode, ops_mode, set_mode, use_hip  # noqa: F401

GEGLU_BLOCK = 16  # row-interleave granularity of packed GEGLU weights


# ----------------------------------------------------------------------------
# GEMM  (Linear / 1x1 conv)
# ----------------------------------------------------------------------------
def pack_geglu(w: torch.Tensor, b: torch.Tensor | None):
    """[2F, K] (hidden rows then gate rows, diffusers GEGLU order) ->
    rows interleaved in blocks of 16: h0..h15, g0..g15, h16..h31, ...
    so one 16-column MFMA output sub-tile pair holds (hidden, gate) for the same
    output columns in the same lane: the GEGLU epilogue needs no shuffle."""
    two_f, k = w.shape
    f = two_f // 2
    assert f % GEGLU_BLOCK == 0
    wp = w.view(2, f // GEGLU_BLOCK, GEGLU_BLOCK, k).transpose(0, 1).reshape(two_f, k)
    bp = None
    if b is not None:
        bp = b.view(2, f // GEGLU_BLOCK, GEGLU_BLOCK).transpose(0, 1).reshape(two_f)
    return wp.contiguous(), (bp.contiguous() if bp is not None else None)


def _gelu_f(x):
    return F.gelu(x)


_ACT_REF = {
    None: lambda y: y, "none": lambda y: y, "gelu": F.gelu, "silu": F.silu,
    "quick_gelu": lambda y: y * torch.sigmoid(1.702 * y), "lrelu": lambda y: F.leaky_relu(y, 0.2),
    "lrelu0.1": lambda y: F.leaky_relu(y, 0.1), "lrelu0.01": lambda y: F.leaky_relu(y, 0.01),
    "tanh": torch.tanh, "relu": F.relu, "elu": F.elu, "gelu_tanh": lambda y: F.gelu(y, approximate="tanh"),
}


def apply_act(y, act):
    """Reference pointwise activation (codes shared with the GEMM/conv epilogue)."""
    return _ACT_REF[act](y)


def _cdt(t):
    """Reference compute dtype: fp32 on CPU; the tensor's own dtype on GPU (so
    ``reference`` mode on MI355X is the diffusers-style bf16 eager baseline:
    hipBLASLt GEMMs, MIOpen channels-last convs, SDPA attention)."""
    return torch.float32 if not t.is_cuda else t.dtype


def _ref_gemm(a2, w, bias, residual, act):
    dt = _cdt(a2)
    if bias is not None:
        y = torch.addmm(bias.to(dt), a2.to(dt), w.to(dt).t())
    else:
        y = a2.to(dt) @ w.to(dt).t()
    if act == "geglu":
        m, n = y.shape
        y = y.view(m, n // (2 * GEGLU_BLOCK), 2, GEGLU_BLOCK)
        y = (y[:, :, 0, :] * _gelu_f(y[:, :, 1, :])).reshape(m, n // 2)
    else:
        y = apply_act(y, act)
    if residual is not None:
        y = y + residual.reshape(y.shape).to(dt)
    return y.to(a2.dtype)


def gemm(a: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act=None, gn_rows=0, row_stats=False):
    """y[..., N'] = act(a[..., K] @ w[N, K]^T + bias) + residual.

    ``act='geglu'`` expects ``pack_geglu`` weights and returns N' = N/2.
    ``gn_rows`` > 0 asks the HIP epilogue for the GroupNorm statistics of the
    output (``gn_rows`` rows per sample) for the GroupNorm that consumes it;
    ``row_stats`` for the per-row statistics a consumer's fused LayerNorm
    (``layer_norm_gemm``) reads."""
    lead = a.shape[:-1]
    k = a.shape[-1]
    a2 = a.reshape(-1, k)
    if use_hip(a):
        from . import hip_ops

        y = hip_ops.gemm(a2, w, bias, residual, act, gn_rows=gn_rows, row_stats=row_stats)
    else:
        y = _ref_gemm(a2, w, bias, residual, act)
    out = y.view(*lead, y.shape[-1])
    for attr in ("_csk_gn", "_csk_rows"):
        st = getattr(y, attr, None)
        if st is not None:
            setattr(out, attr, st)
    return out


def fold_layer_norm(w: torch.Tensor, bias, gamma: torch.Tensor, beta):
    """LayerNorm(x) @ w^T + bias == rstd * (x @ w'^T - mean * colsum) + bias'
    with w' = w * gamma (per input column), colsum = rowsum(w') in fp32 (of the
    bf16-rounded w', so the correction matches what the MFMAs multiply) and
    bias' = bias + w @ beta.  Returns (w', colsum, bias')."""
    wf = w.float()
    w2 = (wf * gamma.float()[None, :]).to(w.dtype)
    colsum = w2.float().sum(1).contiguous()
    b2 = wf @ beta.float() if beta is not None else torch.zeros(w.shape[0], device=w.device)
    if bias is not None:
        b2 = b2 + bias.float()
    return w2.contiguous(), colsum, b2.to(w.dtype)


# On by default since the row-layout direct epilogue carries both halves (the
# producer's per-row sums, the consumer's rstd * (acc - mean * colsum)): one
# MI355X, one process (tools/abstep.py arms lnoff / lnon) 12.79 -> 12.70 ms per
# UNet step (profiles/unet_step_ab_lnfuse_r2x.txt).  With the LDS epilogue it
# had been 0.27-0.6 ms SLOWER than LayerNorm kernels.  CSK_LN_FUSE=0 disables.
LN_FUSE = os.environ.get("CSK_LN_FUSE", "1") == "1"


# CSK_SIDE_STREAM=1: ResNet 1x1 shortcuts run on a side HIP stream forked from /
# joined to the current one (inside a hipGraph capture: a parallel branch) to
# overlap the memory-bound GroupNorm passes of the main path.  Off: the 14
# fork/join pairs per UNet step cost more (cross-queue signals) than the overlap
# gains -- 11.98 vs 11.76 ms/step (tools/abstep.py side0/side1,
# profiles/unet_step_ab_side_r4g.txt)
SIDE_STREAM = os.environ.get("CSK_SIDE_STREAM", "0") == "1"
_SIDE: dict = {}


class side_branch:
    """``with side_branch(x) as br: ...`` runs the block on a side stream of
    x's device (HIP path only; a no-op context elsewhere); ``br.join()`` makes
    the current stream wait for it.  The block's outputs are only used after
    the join, and the side stream waits for everything queued before the fork."""

    def __init__(self, x: torch.Tensor):
        self.on = SIDE_STREAM and use_hip(x)
        self.dev = x.device

    def __enter__(self):
        if self.on:
            self.main = torch.cuda.current_stream(self.dev)
            self.side = _SIDE.get(self.dev)
            if self.side is None:
                self.side = _SIDE[self.dev] = torch.cuda.Stream(self.dev)
            self.side.wait_stream(self.main)
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.on:
            self._ctx.__exit__(*exc)
        return False

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)


def row_stats_wanted(x: torch.Tensor) -> bool:
    """Should a producer GEMM emit row statistics for a LayerNorm consumer?"""
    return LN_FUSE and use_hip(x)


def ln_fusable(x: torch.Tensor) -> bool:
    """x carries the producer's row statistics (HIP path) for ``layer_norm_gemm``."""
    rows = getattr(x, "_csk_rows", None)
    return LN_FUSE and use_hip(x) and rows is not None and x.shape[-1] % 8 == 0


def layer_norm_gemm(x, norm, w, bias, folded, act=None, residual=None, row_stats=False):
    """act(LayerNorm(x) @ w^T + bias) + residual.  On the HIP path with the
    producer's row statistics attached to ``x`` the LayerNorm runs inside the
    GEMM epilogue (``folded`` = fold_layer_norm(w, bias, norm.weight, norm.bias));
    otherwise LayerNorm kernel + GEMM."""
    if ln_fusable(x):
        from . import hip_ops

        w2, colsum, b2 = folded
        lead = x.shape[:-1]
        y = hip_ops.gemm(x.reshape(-1, x.shape[-1]), w2, b2, residual, act,
                         ln=(x._csk_rows, colsum, float(norm.eps)), row_stats=row_stats)
        out = y.view(*lead, y.shape[-1])
        if getattr(y, "_csk_rows", None) is not None:
            out._csk_rows = y._csk_rows
        return out
    return gemm(layer_norm(x, norm.weight, norm.bias, norm.eps), w, bias, residual=residual, act=act,
                row_stats=row_stats)


def qattn_fusable(x: torch.Tensor, kv, rows_per_b: int) -> bool:
    """The query projection of this cross-attention can carry the attention in
    its epilogue (HIP path; head dim 64, <= 80 context tokens)."""
    if not use_hip(x):
        return False
    from . import hip_ops

    return hip_ops.qattn_ok(x, kv, rows_per_b)


def layer_norm_gemm_attn(x, norm, w, bias, folded, kv, scale, rows_per_b):
    """softmax((LayerNorm(x) @ w^T + bias) K^T * scale) V over the per-request
    ``kv`` [B, Skv, 2, H, D] (the attention output before the out-projection),
    the attention running in the query projection's epilogue on the HIP path."""
    lead = x.shape[:-1]
    if use_hip(x):
        from . import hip_ops

        if ln_fusable(x):
            w2, colsum, b2 = folded
            o = hip_ops.gemm_attn(x.reshape(-1, x.shape[-1]), w2, b2, kv, scale, rows_per_b,
                                  ln=(x._csk_rows, colsum, float(norm.eps)))
        else:
            xn = layer_norm(x, norm.weight, norm.bias, norm.eps)
            o = hip_ops.gemm_attn(xn.reshape(-1, x.shape[-1]), w, bias, kv, scale, rows_per_b)
        return o.view(*lead, o.shape[-1])
    return _ref_gemm_attn(layer_norm(x, norm.weight, norm.bias, norm.eps), w, bias, kv, scale)


def _ref_gemm_attn(xn, w, bias, kv, scale):
    """fp32 reference: q = xn @ w^T + bias, softmax(q K^T * scale) V per head."""
    b, s, c = xn.shape
    q = xn.float() @ w.float().t()
    if bias is not None:
        q = q + bias.float()
    heads, d = kv.shape[3], kv.shape[4]
    k, v = kv[:b, :, 0].float(), kv[:b, :, 1].float()
    qh = q.view(b, s, heads, d).transpose(1, 2)
    att = torch.softmax((qh @ k.permute(0, 2, 3, 1)) * scale, -1)
    return (att @ v.transpose(1, 2)).transpose(1, 2).reshape(b, s, c).to(xn.dtype)


# the 16-column block order of the fused FF's W2 (csrc/kernels/ff.hip: a lane's
# 8 GEGLU results are intermediates {4h + j, 8 + 4h + j})
_FF_PERM = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def _ff_keys(device):
    """16-byte chunk swizzles of the fused FF's LDS images (ff.hip): a W1
    sub-image row r [32][64] holds logical chunk pos ^ ((r & 7) ^ ((r >> 3) & 1))
    at position pos; a W2 tile row [32][32], pos ^ ((r >> 2) & 3)."""
    r = torch.arange(32, device=device)
    k1 = (r & 7) ^ ((r >> 3) & 1)
    k2 = (r >> 2) & 3
    p8, p4 = torch.arange(8, device=device), torch.arange(4, device=device)
    return p8[None, :] ^ k1[:, None], p4[None, :] ^ k2[:, None]  # [32, 8], [32, 4]


def pack_ff_fused(w1, b1, w2):
    """Weights of the fused feed-forward kernel from the diffusers GEGLU
    projection ``w1`` [2I, C] (+ ``b1`` [2I]; value rows first, gate rows second)
    and the down-projection ``w2`` [C, I], laid out in global memory exactly as
    the kernel's LDS images (swizzle included), so every LDS-DMA piece is one
    contiguous 1 KB run:
      w1p [I/16, C/64, 32, 64]: W1 tile t = 16 value rows + the 16 gate rows of
          intermediates 16t.., as C/64 swizzled [32][64] sub-images;
      b1p [I/16, 32] fp32 (same row order);
      w2p [I/32, C/32, 32, 32]: per 32 intermediates, one swizzled [32][32]
          image per 32 output rows, columns in 16-blocks ordered 0-3, 8-11, 4-7, 12-15."""
    two_i, c = w1.shape
    inner = two_i // 2
    t = inner // 16
    k8, k4 = _ff_keys(w1.device)
    w1t = torch.stack((w1[:inner].reshape(t, 16, c), w1[inner:].reshape(t, 16, c)), 1).reshape(t, 32, c // 64, 8, 8)
    w1p = torch.gather(w1t, 3, k8[None, :, None, :, None].expand(t, 32, c // 64, 8, 8))  # pos <- logical chunk
    w1p = w1p.permute(0, 2, 1, 3, 4).reshape(t, c // 64, 32, 64)
    b1p = None
    if b1 is not None:
        b1p = torch.stack((b1[:inner].reshape(t, 16), b1[inner:].reshape(t, 16)), 1).reshape(t, 32).float()
    return w1p.contiguous(), (None if b1p is None else b1p.contiguous()), _pack_ff_w2(w2)


def _pack_ff_w2(w2):
    """[C, K] -> [K/32, C/32, 32, 32]: per 32 input columns one swizzled [32][32]
    image per 32 output rows, columns in 16-blocks ordered ``_FF_PERM``."""
    c, inner = w2.shape
    _, k4 = _ff_keys(w2.device)
    perm = torch.tensor(_FF_PERM, device=w2.device)
    w2q = w2.reshape(c, inner // 16, 16).index_select(2, perm).reshape(c // 32, 32, inner // 32, 4, 8)
    w2p = torch.gather(w2q, 3, k4[None, :, None, :, None].expand(c // 32, 32, inner // 32, 4, 8))
    return w2p.permute(2, 0, 1, 3, 4).reshape(inner // 32, c // 32, 32, 32).contiguous()


def _unpack_ff_w2(w2p):
    nc, no = w2p.shape[0], w2p.shape[1]
    c, inner = 32 * no, 32 * nc
    _, k4 = _ff_keys(w2p.device)
    inv4 = torch.argsort(k4, 1)
    y = w2p.reshape(nc, no, 32, 4, 8).permute(1, 2, 0, 3, 4)  # [o, r, c, pos, e]
    y = torch.gather(y, 3, inv4[None, :, None, :, None].expand(no, 32, nc, 4, 8)).reshape(c, inner // 16, 16)
    return y[:, :, torch.argsort(torch.tensor(_FF_PERM, device=w2p.device))].reshape(c, inner)


def unpack_ff_fused(w1p, b1p, w2p):
    """Inverse of ``pack_ff_fused``: (w1 [2I, C], b1 [2I] or None, w2 [C, I])."""
    t, si = w1p.shape[0], w1p.shape[1]
    c, inner = 64 * si, 16 * t
    k8, _ = _ff_keys(w1p.device)
    inv8 = torch.argsort(k8, 1)
    x = w1p.reshape(t, si, 32, 8, 8).permute(0, 2, 1, 3, 4)  # [t, r, si, pos, e]
    x = torch.gather(x, 3, inv8[None, :, None, :, None].expand(t, 32, si, 8, 8)).reshape(t, 32, c)
    w1 = torch.cat((x[:, :16].reshape(inner, c), x[:, 16:].reshape(inner, c)), 0)
    b1 = None if b1p is None else torch.cat((b1p[:, :16].reshape(inner), b1p[:, 16:].reshape(inner)), 0)
    return w1, b1, _unpack_ff_w2(w2p)


def ff_fusable(x: torch.Tensor, inner: int) -> bool:
    """The fused feed-forward kernel takes this block (HIP path, C = 320)."""
    if not use_hip(x) or x.dim() != 3:
        return False
    from . import hip_ops

    return hip_ops.ff_fused_ok(x, inner)


def ff_fused(x, gamma, beta, w1p, b1p, w2p, b2, eps):
    """x + FF(LayerNorm(x)) with a GEGLU feed-forward; one HIP kernel, or the
    fp32 reference composition of the packed weights."""
    if use_hip(x):
        from . import hip_ops

        return hip_ops.ff_geglu(x, gamma, beta, w1p, b1p, w2p, b2, eps)
    return _ref_ff_fused(x, gamma, beta, w1p, b1p, w2p, b2, eps)


def _ref_ff_fused(x, gamma, beta, w1p, b1p, w2p, b2, eps):
    """fp32 reference from the packed weights (unpacks them): LayerNorm, GEGLU
    with the exact GELU, down-projection, bias, residual."""
    w1, b1, w2 = unpack_ff_fused(w1p, b1p, w2p)
    c, inner = w2.shape
    xf = x.float()
    h = torch.nn.functional.layer_norm(xf, (c,), gamma.float(), None if beta is None else beta.float(), eps)
    vg = torch.nn.functional.linear(h, w1.float(), None if b1 is None else b1.float())
    hid = vg[..., :inner] * torch.nn.functional.gelu(vg[..., inner:])
    y = torch.nn.functional.linear(hid, w2.float(), None if b2 is None else b2.float())
    return (xf + y).to(x.dtype)


def pack_ff_proj(wp):
    """The transformer's ``proj_out`` weight [C, C] for the tail of the fused
    feed-forward (ff.hip, PROJ variant): packed exactly like its W2, the FF
    output's channels taking the place of the intermediates: [C/32, C/32, 32, 32]."""
    c = wp.shape[0]
    return _pack_ff_w2(wp.reshape(c, c))


def unpack_ff_proj(wpp):
    """Inverse of ``pack_ff_proj``: [C, C]."""
    return _unpack_ff_w2(wpp)


def ff_proj_fusable(x: torch.Tensor, inner: int, gn_rows: int) -> int:
    """GroupNorm segment height (non-zero) when the fused feed-forward also
    takes the transformer's proj_out for this block (HIP path, C = 320, whole
    128-row tiles), else 0."""
    if not use_hip(x) or x.dim() != 3:
        return 0
    from . import hip_ops

    return hip_ops.ff_proj_ok(x, inner, gn_rows)


def ff_fused_proj(x, gamma, beta, w1p, b1p, w2p, b2, wpp, bp, xin, eps, gn_rows=0, seg=0):
    """xin + proj_out(x + FF(LayerNorm(x))), shaped like ``xin``: one HIP kernel
    (with the GroupNorm partials of the result when ``seg`` > 0), or the fp32
    reference composition of the packed weights."""
    if use_hip(x):
        from . import hip_ops

        return hip_ops.ff_geglu_proj(x, gamma, beta, w1p, b1p, w2p, b2, wpp, bp, xin, eps, gn_rows, seg)
    return _ref_ff_fused_proj(x, gamma, beta, w1p, b1p, w2p, b2, wpp, bp, xin, eps)


def _ref_ff_fused_proj(x, gamma, beta, w1p, b1p, w2p, b2, wpp, bp, xin, eps):
    """fp32 reference from the packed weights: ``_ref_ff_fused`` (kept in fp32),
    then the projection, its bias and the residual ``xin``."""
    wp = unpack_ff_proj(wpp)
    y = _ref_ff_fused(x.float(), gamma, beta, w1p, b1p, w2p, b2, eps)
    z = torch.nn.functional.linear(y, wp.float(), None if bp is None else bp.float())
    return (xin.float() + z.reshape(xin.shape)).to(x.dtype)


def _a_tiles(w):
    """[N, C] (N % 32 == 0, C % 64 == 0) -> the 32x32x16 A-operand LDS images
    [N/32, C/64, 32, 64] of ff.hip / xin.hip: row r of a sub-image holds
    logical 16-byte chunk c at position c ^ ((r & 7) ^ ((r >> 3) & 1))."""
    n, c = w.shape
    t = n // 32
    k8, _ = _ff_keys(w.device)
    x = w.reshape(t, 32, c // 64, 8, 8)
    x = torch.gather(x, 3, k8[None, :, None, :, None].expand(t, 32, c // 64, 8, 8))
    return x.permute(0, 2, 1, 3, 4).reshape(t, c // 64, 32, 64)


def _a_untiles(p):
    t, si = p.shape[0], p.shape[1]
    k8, _ = _ff_keys(p.device)
    inv8 = torch.argsort(k8, 1)
    x = p.reshape(t, si, 32, 8, 8).permute(0, 2, 1, 3, 4)
    return torch.gather(x, 3, inv8[None, :, None, :, None].expand(t, 32, si, 8, 8)).reshape(32 * t, 64 * si)


def pack_xin_qkv(wi, bi, wq, colsum, bq):
    """Weights of the fused transformer-input kernel (xin.hip) from proj_in
    ``wi`` [C, C] (+ ``bi``) and the LN1-folded QKV projection (``wq`` [3C, C],
    ``colsum``, ``bq`` from ``fold_layer_norm``): one bf16 buffer of the 10 + 30
    A-operand tiles as their LDS images, Wqkv's columns permuted within every
    16-block to the order the proj_in accumulators hand over (0-3, 8-11, 4-7,
    12-15), and the fp32 tables (bi, colsum, bq)."""
    c = wi.shape[0]
    perm = torch.tensor(_FF_PERM, device=wq.device)
    wqp = wq.reshape(wq.shape[0], c // 16, 16).index_select(2, perm).reshape(wq.shape[0], c)
    w = torch.cat([_a_tiles(wi.reshape(c, c)), _a_tiles(wqp)], 0).contiguous()
    f32 = lambda t, n: (torch.zeros(n, device=wi.device) if t is None else t.float()).contiguous()  # noqa: E731
    return w, f32(bi, c), f32(colsum, wq.shape[0]), f32(bq, wq.shape[0])


def unpack_xin_qkv(w):
    """Inverse of ``pack_xin_qkv``'s weight buffer: (wi [C, C], wq [3C, C])."""
    c = 64 * w.shape[1]
    full = _a_untiles(w)
    wi, wqp = full[:c], full[c:]
    inv = torch.argsort(torch.tensor(_FF_PERM, device=w.device))
    return wi, wqp.reshape(wqp.shape[0], c // 16, 16).index_select(2, inv).reshape(wqp.shape[0], c)


def xin_fusable(x: torch.Tensor, groups: int) -> bool:
    """The fused transformer-input kernel takes this block input (HIP path,
    C = 320, the producer's GroupNorm statistics attached)."""
    if not use_hip(x):
        return False
    from . import hip_ops

    return hip_ops.xin_ok(x, groups)


def xin_qkv(x, gn_gamma, gn_beta, groups, gn_eps, packed, ln_eps):
    """(h, qkv): h = proj_in(GroupNorm(x)), qkv = LayerNorm1(h) Wqkv^T + b with
    the LN1 affine folded into ``packed`` (``pack_xin_qkv``).  x: [B, ..., C];
    h [M, C], qkv [M, 3C].  One HIP kernel (None when the producer's
    statistics are missing), or the fp32 reference composition."""
    w, bi, colsum, bq = packed
    if use_hip(x):
        from . import hip_ops

        stat = hip_ops.gn_stats(x, groups, gn_eps)
        if stat is None:
            return None
        return hip_ops.xin_qkv(x, stat, gn_gamma, gn_beta, w, bi, colsum, bq, ln_eps)
    return _ref_xin_qkv(x, gn_gamma, gn_beta, groups, gn_eps, packed, ln_eps)


def _ref_xin_qkv(x, gn_gamma, gn_beta, groups, gn_eps, packed, ln_eps):
    """fp32 reference from the packed weights: GroupNorm, proj_in, LayerNorm
    (affine folded into the weights), QKV projection."""
    w, bi, colsum, bq = packed
    wi, wq = unpack_xin_qkv(w)
    B, C = x.shape[0], x.shape[-1]
    xf = x.float().reshape(B, -1, C)
    g = xf.reshape(B, -1, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = g.var(dim=(1, 3), keepdim=True, unbiased=False)
    xg = ((g - mean) * torch.rsqrt(var + gn_eps)).reshape(B, -1, C)
    xg = xg * gn_gamma.float() + (0 if gn_beta is None else gn_beta.float())
    h = xg @ wi.float().t() + bi
    n = torch.nn.functional.layer_norm(h, (C,), eps=ln_eps)
    qkv = n @ wq.float().t() + bq
    return h.reshape(-1, C).to(x.dtype), qkv.reshape(-1, 3 * C).to(x.dtype)


def xattn_fusable(x: torch.Tensor, kv, rows_per_b: int) -> bool:
    """The fused cross-attention sub-block kernel takes this block (HIP path)."""
    if not use_hip(x):
        return False
    from . import hip_ops

    return hip_ops.xattn_ok(x, kv, rows_per_b)


# column order of the folded query weight for the fused block's prologue
# variant (csrc/kernels/xattn.hip PRE): within each 32-column block, position
# 8 g + j holds column 4 g + j (j < 4) or 16 + 4 g + j - 4 (the k-slot order in
# which the prologue's accumulators arrive)
_XQ_PERM = tuple((4 * g + j if j < 4 else 16 + 4 * g + j - 4) for g in range(4) for j in range(8))


def permute_xattn_q(wq):
    """Folded query weight [N, C] (C % 32 == 0) with its columns in the
    prologue variant's order; ``colsum`` and the bias are unaffected."""
    n, c = wq.shape
    return wq.reshape(n, c // 32, 32)[:, :, torch.tensor(_XQ_PERM, device=wq.device)].reshape(n, c).contiguous()


def unpermute_xattn_q(wqp):
    """Inverse of ``permute_xattn_q``."""
    n, c = wqp.shape
    inv = torch.argsort(torch.tensor(_XQ_PERM, device=wqp.device))
    return wqp.reshape(n, c // 32, 32)[:, :, inv].reshape(n, c).contiguous()


def xattn_pre_fusable(o: torch.Tensor, kv, rows_per_b: int, dup=False) -> bool:
    """The fused cross-attention sub-block also takes the preceding
    out-projection of the attention output ``o`` as its prologue (``dup``: for
    both CFG halves from the one half in ``o``)."""
    if not use_hip(o):
        return False
    from . import hip_ops

    return hip_ops.xattn_pre_ok(o, kv, rows_per_b, dup)


def xattn_block(x, wq, colsum, bq, kv, wo, bo, eps, scale, rows_per_b, row_stats=True, pre=None, batch=None):
    """x + CrossAttention(LayerNorm(x)) with the LayerNorm folded into ``wq`` /
    ``colsum`` / ``bq`` (fold_layer_norm) and ``kv`` the per-request K/V
    [B, Skv, 2, H, D]; one HIP kernel, or the reference composition.
    ``pre = (o, h0, wo1, bo1)`` with ``x`` None: x = h0 + o wo1^T + bo1, the
    out-projection of the preceding attention, is formed inside (``wq`` then
    ``permute_xattn_q``'d), for ``batch`` samples (a multiple of ``o``'s, which
    then repeats)."""
    if use_hip(x if pre is None else pre[0]):
        from . import hip_ops

        return hip_ops.xattn_block(x, wq, colsum, bq, kv, wo, bo, eps, scale, rows_per_b, row_stats=row_stats,
                                   pre=pre, batch=batch)
    return _ref_xattn_block(x, wq, colsum, bq, kv, wo, bo, eps, scale, pre=pre, batch=batch)


def _ref_xattn_block(x, wq, colsum, bq, kv, wo, bo, eps, scale, pre=None, batch=None):
    """fp32 reference: LN(x) @ Wq^T from the folded form (== the unfolded LN +
    projection), softmax attention over kv, out-projection, residual.  With
    ``pre``: x from the out-projection (fp32), ``wq`` un-permuted."""
    if pre is not None:
        o, h0, wo1, bo1 = pre
        xf = h0.float() + o.float() @ wo1.float().t()
        if bo1 is not None:
            xf = xf + bo1.float()
        if batch is not None and batch != o.shape[0]:
            xf = xf.repeat(batch // o.shape[0], 1, 1)
        dt, x, wq = o.dtype, xf, unpermute_xattn_q(wq)
    else:
        dt = x.dtype
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    rstd = torch.rsqrt(xf.var(-1, unbiased=False, keepdim=True) + eps)
    q = rstd * (xf @ wq.float().t() - mean * colsum.float()) + bq.float()
    b, s, c = x.shape
    heads, d = kv.shape[3], kv.shape[4]
    k, v = kv[:b, :, 0].float(), kv[:b, :, 1].float()  # [B, Skv, H, D]
    qh = q.view(b, s, heads, d).transpose(1, 2)
    att = torch.softmax((qh @ k.permute(0, 2, 3, 1)) * scale, -1)
    o = (att @ v.transpose(1, 2)).transpose(1, 2).reshape(b, s, c)
    y = o @ wo.float().t() + xf
    if bo is not None:
        y = y + bo.float()
    return y.to(dt)


def cat_channels(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat on the channel (last) dim that keeps fused GroupNorm
    statistics: they are per (row tile, channel), so the concatenated tensor's
    statistics are the two parts side by side (UNet skip connections)."""
    y = torch.cat([a, b], dim=-1)
    sa, sb = getattr(a, "_csk_gn", None), getattr(b, "_csk_gn", None)
    if sa is not None and sb is not None and sa[1] == sb[1]:
        ca, cb = a.shape[-1], b.shape[-1]
        nseg = sa[0].numel() // (2 * ca)
        if nseg * 2 * cb == sb[0].numel():
            y._csk_gn = (torch.cat([sa[0].view(nseg, ca, 2), sb[0].view(nseg, cb, 2)], 1).view(-1), sa[1])
    return y


# ----------------------------------------------------------------------------
# Conv2d NHWC (implicit GEMM)
# ----------------------------------------------------------------------------
def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, kh, kw] (PyTorch/diffusers) -> [Cout, kh, kw, Cin]."""
    return w.permute(0, 2, 3, 1).contiguous()


def norm_padding(padding):
    """int p -> (top, left, bottom, right)."""
    if isinstance(padding, int):
        return (padding,) * 4
    assert len(padding) == 4
    return tuple(int(p) for p in padding)


def conv_out_size(h, w, kh, kw, stride, padding, up2x=False, dilation=1):
    pt, pl, pb, pr = norm_padding(padding)
    if up2x:
        h, w = 2 * h, 2 * w
    return ((h + pt + pb - dilation * (kh - 1) - 1) // stride + 1,
            (w + pl + pr - dilation * (kw - 1) - 1) // stride + 1)


def _ref_conv2d(x, wp, bias, stride, padding, residual, up2x, bias2d, act=None, out_scale=1.0, dilation=1,
                residual2=None, res_scale=1.0, extra=None):
    dt = _cdt(x)
    # NHWC tensor viewed as channels-last NCHW: no copies, MIOpen NHWC kernels
    xn = x.to(dt).permute(0, 3, 1, 2)
    if up2x:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    pt, pl, pb, pr = norm_padding(padding)
    w = wp.to(dt).permute(0, 3, 1, 2)
    b = bias.to(dt) if bias is not None else None
    if pt == pb and pl == pr and min(pt, pl) >= 0:
        y = F.conv2d(xn, w, b, stride=stride, padding=(pt, pl), dilation=dilation)
    else:
        y = F.conv2d(F.pad(xn, (pl, pr, pt, pb)), w, b, stride=stride, dilation=dilation)
    y = y.permute(0, 2, 3, 1)
    for a, wa in extra or ():
        y = y + a.to(dt) @ wa.to(dt).t()
    if bias2d is not None:
        y = y + bias2d.to(dt)[:, None, None, :]
    y = apply_act(y, act)
    if out_scale != 1.0:
        y = y * out_scale
    if residual is not None:
        y = y + (residual.to(dt) if res_scale == 1.0 else res_scale * residual.to(dt))
    if residual2 is not None:
        y = y + residual2.to(dt)
    return y.to(x.dtype).contiguous()


# A ResNet's 1x1 shortcut folded into its conv2 as extra K segments
# (conv2d(extra=...)); CSK_SC_FUSE=0: the shortcut stays its own GEMM(s) and
# conv2 adds it as a residual
SC_FUSE = os.environ.get("CSK_SC_FUSE", "1") == "1"


def pack_conv_extra(wp: torch.Tensor, ws) -> tuple:
    """One [Cout, kh*kw*Cin + sum Ci] K-contiguous matrix from a packed conv
    weight [Cout, kh, kw, Cin] and the [Cout, Ci] weights of its extra K
    segments.  Returns (matrix, conv view [Cout, kh, kw, Cin], segment views):
    the views are what ``conv2d(..., extra=...)`` takes."""
    cout, kh, kw, cin = wp.shape
    wf = torch.cat([wp.reshape(cout, -1)] + [w.reshape(cout, -1).to(wp.dtype) for w in ws], dim=1).contiguous()
    k0, views = kh * kw * cin, []
    off = k0
    for w in ws:
        c = w.reshape(cout, -1).shape[1]
        views.append(wf[:, off:off + c])
        off += c
    return wf, wf[:, :k0].unflatten(1, (kh, kw, cin)), tuple(views)


def conv_extra_fusable(x, wp, extra, stride=1, padding=1, up2x=False, dilation=1) -> bool:
    """``conv2d(..., extra=extra)`` is available for this call: always on the
    plain-PyTorch path, on the HIP path under the kernels' conditions
    (``hip_ops.conv_extra_ok``)."""
    if not use_hip(x):
        return True
    from . import hip_ops

    return hip_ops.conv_extra_ok(x, wp, extra, stride, padding, up2x, dilation)


def conv2d(x, wp, bias=None, stride=1, padding=1, residual=None, up2x=False, bias2d=None, act=None,
           out_scale=1.0, out=None, dilation=1, gn_stats=False, residual2=None, res_scale=1.0, out_u8=False,
           norm=None, norm_optional=False, extra=None):
    """NHWC conv.  ``wp``: packed [Cout, kh, kw, Cin].  ``up2x`` fuses a
    nearest-neighbour x2 upsample into the input addressing; ``bias2d`` [B, Cout]
    is a per-sample channel bias (ResNet time-embedding add) fused in the
    epilogue; y = act(conv + bias + bias2d) * out_scale + residual.  ``x``,
    ``residual`` and ``out`` may be channel slices of wider NHWC buffers.
    ``gn_stats``: the HIP epilogue also emits the GroupNorm statistics of the
    output (consumed by ``group_norm`` of that tensor; skips its stats pass).
    ``residual2`` / ``res_scale``: y = act(...) * out_scale + res_scale *
    residual + residual2 (Real-ESRGAN's nested "* 0.2 + x" in one epilogue;
    ``out`` may alias ``residual2``).  ``out_u8``: the output is a uint8 image,
    round(clamp(y, 0, 1) * 255) (Real-ESRGAN's RGB conv_last).
    ``norm = (gamma, beta, groups, eps, silu, keep_raw)``: the GroupNorm that
    consumes the output, i.e. ``group_norm(conv2d(...), gamma, beta, groups, eps,
    silu)``; the call returns the normalised tensor, or (normalised, raw) with
    ``keep_raw`` (``out=``, the raw output's buffer, needs it).  A split-K plan on the HIP path applies it in the reduce
    kernel, so the raw tensor is never written unless kept.  ``norm_optional``
    (with ``keep_raw``): apply the norm only where it costs no extra kernel,
    else return (None, raw) and leave it to the consumer of the raw tensor.
    ``extra = ((a, wa), (b, wb))`` (one or two pairs): extra K segments,
    y = act(conv(x) + a . wa^T + b . wb^T + bias + bias2d) * out_scale + residual
    with ``a`` / ``b`` NHWC [B, Ho, Wo, Ci] and ``wa`` / ``wb`` [Cout, Ci]; the
    HIP path runs them inside the conv's K loop and needs ``wp`` and the
    segment weights to come from ``pack_conv_extra`` (``conv_extra_fusable``)."""
    if use_hip(x):
        from . import hip_ops

        return hip_ops.conv2d(x, wp, bias, stride, padding, residual, up2x, bias2d, act, out_scale, out, dilation,
                              gn_stats, residual2=residual2, res_scale=res_scale, out_u8=out_u8, norm=norm,
                              norm_optional=norm_optional, extra=extra)
    if norm is not None and (out_u8 or residual2 is not None or res_scale != 1.0):
        raise ValueError("conv2d: norm with out_u8 / residual2 / res_scale")
    if norm is not None and out is not None and not norm[5]:
        raise ValueError("conv2d: out= with norm is the raw output: it needs keep_raw")
    y = _ref_conv2d(x, wp, bias, stride, padding, residual, up2x, bias2d, act, out_scale, dilation,
                    residual2, res_scale, extra)
    if out_u8:
        y = (y.float().clamp(0, 1) * 255).round().to(torch.uint8)
    if out is not None:
        out.copy_(y)
        y = out
    if norm is not None:
        gamma, beta, groups, eps, silu, keep_raw = norm
        if norm_optional and keep_raw:
            return None, y
        yn = _ref_group_norm(y, gamma, beta, groups, eps, silu)
        return (yn, y) if keep_raw else yn
    return y


# ----------------------------------------------------------------------------
# Depthwise conv2d NHWC (K-UNet binomial resamplers, ConvNeXt 7x7)
# ----------------------------------------------------------------------------
DW_KMAX = 7  # largest depthwise kernel side (csrc/kernels/dwconv.hip DW_KMAX)
DW_PAD_MODES = ("zeros", "reflect")


def pack_depthwise_weight(w: torch.Tensor) -> torch.Tensor:
    """[C, 1, kh, kw] (PyTorch depthwise) or [C, kh, kw] -> fp32 [kh, kw, C]."""
    if w.dim() == 4:
        if w.shape[1] != 1:
            raise ValueError(f"pack_depthwise_weight: expected [C, 1, kh, kw], got {tuple(w.shape)}")
        w = w[:, 0]
    if w.dim() != 3:
        raise ValueError(f"pack_depthwise_weight: expected [C, 1, kh, kw] or [C, kh, kw], got {tuple(w.shape)}")
    return w.detach().permute(1, 2, 0).float().contiguous()


def _dw_check(name, x, wp, bias, padding, pad_mode):
    """Validation shared by the reference and the HIP path of the depthwise ops;
    returns (pt, pl, pb, pr)."""
    if x.dim() != 4:
        raise ValueError(f"{name}: x must be NHWC [B, H, W, C], got {tuple(x.shape)}")
    B, H, W, C = x.shape
    if C % 8 != 0:
        raise ValueError(f"{name}: C = {C} is not a multiple of 8")
    if wp.dim() != 3 or wp.shape[2] != C or wp.dtype != torch.float32:
        raise ValueError(f"{name}: wp must be pack_depthwise_weight's fp32 [kh, kw, {C}], got "
                         f"{wp.dtype} {tuple(wp.shape)}")
    kh, kw = wp.shape[0], wp.shape[1]
    if not (1 <= kh <= DW_KMAX and 1 <= kw <= DW_KMAX):
        raise ValueError(f"{name}: kernel {kh}x{kw} outside 1..{DW_KMAX}")
    if pad_mode not in DW_PAD_MODES:
        raise ValueError(f"{name}: pad_mode {pad_mode!r} not in {DW_PAD_MODES}")
    pad = norm_padding(padding)
    if min(pad) < 0:
        raise ValueError(f"{name}: negative padding {pad}")
    pt, pl, pb, pr = pad
    if pad_mode == "reflect" and (max(pt, pb) >= H or max(pl, pr) >= W):
        raise ValueError(f"{name}: reflect padding {pad} must be smaller than the input {H}x{W}")
    if bias is not None and tuple(bias.shape) != (C,):
        raise ValueError(f"{name}: bias shape {tuple(bias.shape)} != ({C},)")
    return pad


def _dw_view_check(name, t, shape, what):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {what} shape {tuple(t.shape)} != {tuple(shape)}")


def _dw_padded(x, pad, pad_mode):
    """NCHW view of NHWC ``x`` in the reference compute dtype, explicitly padded."""
    pt, pl, pb, pr = pad
    xn = x.to(_cdt(x)).permute(0, 3, 1, 2)
    if max(pad) == 0:
        return xn
    return F.pad(xn, (pl, pr, pt, pb), mode="reflect" if pad_mode == "reflect" else "constant")


def _ref_depthwise_conv2d(x, wp, bias, stride, pad, pad_mode, residual):
    dt = _cdt(x)
    c = x.shape[-1]
    w = wp.permute(2, 0, 1).unsqueeze(1).to(dt).contiguous()  # [C, 1, kh, kw]
    y = F.conv2d(_dw_padded(x, pad, pad_mode), w, bias.to(dt) if bias is not None else None, stride=stride, groups=c)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.to(dt)
    return y.to(x.dtype).contiguous()


def depthwise_conv2d(x, wp, bias=None, stride=1, padding=0, pad_mode="zeros", residual=None, out=None):
    """Depthwise NHWC conv: y[b, oh, ow, c] = bias[c] + sum_ij wp[i, j, c] *
    xp[b, oh*s + i, ow*s + j, c] (+ residual), ``xp`` = ``x`` padded by
    ``padding`` (int or (top, left, bottom, right)) with zeros or by reflection
    (``F.pad(mode="reflect")``).  ``wp``: ``pack_depthwise_weight`` fp32
    [kh, kw, C], kh, kw <= 7; stride 1 or 2; C % 8 == 0.  ``x``, ``residual``
    and ``out`` may be channel slices of wider NHWC buffers."""
    name = "depthwise_conv2d"
    pad = _dw_check(name, x, wp, bias, padding, pad_mode)
    if stride not in (1, 2):
        raise ValueError(f"{name}: stride {stride} not in (1, 2)")
    B, H, W, C = x.shape
    ho, wo = conv_out_size(H, W, wp.shape[0], wp.shape[1], stride, pad)
    if ho < 1 or wo < 1:
        raise ValueError(f"{name}: kernel {wp.shape[0]}x{wp.shape[1]} larger than the padded input")
    _dw_view_check(name, residual, (B, ho, wo, C), "residual")
    _dw_view_check(name, out, (B, ho, wo, C), "out")
    if use_hip(x):
        from . import hip_ops

        return hip_ops.depthwise_conv2d(x, wp, bias, stride, pad, pad_mode, residual, out, (ho, wo))
    y = _ref_depthwise_conv2d(x, wp, bias, stride, pad, pad_mode, residual)
    if out is not None:
        out.copy_(y)
        y = out
    return y


def _ref_depthwise_conv_transpose2d(x, wp, bias, pad, pad_mode, crop):
    dt = _cdt(x)
    c = x.shape[-1]
    w = wp.permute(2, 0, 1).unsqueeze(1).to(dt).contiguous()
    y = F.conv_transpose2d(_dw_padded(x, pad, pad_mode), w, bias.to(dt) if bias is not None else None, stride=2,
                           padding=crop, groups=c)
    return y.permute(0, 2, 3, 1).to(x.dtype).contiguous()


def depthwise_conv_transpose2d(x, wp, bias=None, in_padding=0, pad_mode="zeros", crop=0, out=None):
    """Stride-2 depthwise transposed conv on NHWC:
    ``conv_transpose2d(pad(x, in_padding, pad_mode), w, stride=2, padding=crop,
    groups=C)``; output side ``(H + pt + pb - 1) * 2 - 2 * crop + kh``.  The HIP
    kernel gathers (each output pixel sums the taps of its parity) and never
    builds the padded tensor."""
    name = "depthwise_conv_transpose2d"
    pad = _dw_check(name, x, wp, bias, in_padding, pad_mode)
    if not isinstance(crop, int) or crop < 0:
        raise ValueError(f"{name}: crop {crop!r} must be a non-negative int")
    B, H, W, C = x.shape
    pt, pl, pb, pr = pad
    ho = (H + pt + pb - 1) * 2 - 2 * crop + wp.shape[0]
    wo = (W + pl + pr - 1) * 2 - 2 * crop + wp.shape[1]
    if ho < 1 or wo < 1:
        raise ValueError(f"{name}: crop {crop} leaves no output")
    _dw_view_check(name, out, (B, ho, wo, C), "out")
    if use_hip(x):
        from . import hip_ops

        return hip_ops.depthwise_conv_transpose2d(x, wp, bias, pad, pad_mode, crop, out, (ho, wo))
    y = _ref_depthwise_conv_transpose2d(x, wp, bias, pad, pad_mode, crop)
    if out is not None:
        out.copy_(y)
        y = out
    return y


# ----------------------------------------------------------------------------
# 1-D convolutions on token-layout tensors [B, T, C] (HiFi-GAN / EnCodec)
# ----------------------------------------------------------------------------
def conv1d(x, wp, bias=None, padding=0, dilation=1, act=None, residual=None, out_scale=1.0, out=None):
    """x [B, T, Cin], packed wp [Cout, 1, k, Cin] -> [B, T', Cout]: the 2-D
    implicit-GEMM conv on the [B, 1, T, C] view.  ``padding`` int or (left, right)."""
    pl, pr = (padding, padding) if isinstance(padding, int) else padding
    x4 = x.unsqueeze(1)
    r4 = residual.unsqueeze(1) if residual is not None else None
    o4 = out.unsqueeze(1) if out is not None else None
    y = conv2d(x4, wp, bias, 1, (0, pl, 0, pr), residual=r4, act=act, out_scale=out_scale, out=o4,
               dilation=dilation)
    return y.squeeze(1)


def pack_conv_transpose1d(w: torch.Tensor, stride: int, padding: int):
    """Polyphase decomposition of ConvTranspose1d weight [Cin, Cout, k].

    Output sample o = t*s + r only meets taps j = j0 + m*s with
    j0 = (r + p) mod s, reading input t + q - m (q = (r + p) div s).  Each phase
    r is therefore an ordinary correlation with nt = ceil((k - j0)/s) taps and
    left padding nt - 1 - q, written straight into the interleaved output via
    its pixel stride: no zero-insertion, s-fold fewer MACs than the upsample +
    conv formulation.  Returns [(wp_r [Cout, 1, nt, Cin] or None, pl_r)] * s."""
    cin, cout, k = w.shape
    s, p = int(stride), int(padding)
    phases = []
    for r in range(s):
        j0, q = (r + p) % s, (r + p) // s
        nt = max(0, -(-(k - j0) // s))
        if nt == 0:
            phases.append((None, 0))
            continue
        taps = [j0 + (nt - 1 - u) * s for u in range(nt)]
        wr = w[:, :, taps]  # [Cin, Cout, nt]
        phases.append((wr.permute(1, 2, 0).unsqueeze(1).contiguous(), nt - 1 - q))
    return phases


def conv_transpose1d(x, w, bias, stride, padding, phases=None, act=None):
    """x [B, L, Cin] -> [B, (L-1)*s - 2p + k, Cout] (PyTorch ConvTranspose1d
    semantics, weight [Cin, Cout, k]).  ``act`` is applied to the output."""
    b, L, _ = x.shape
    cout, k = w.shape[1], w.shape[2]
    s = int(stride)
    lout = (L - 1) * s - 2 * padding + k
    if not use_hip(x):
        dt = _cdt(x)
        y = F.conv_transpose1d(x.to(dt).transpose(1, 2), w.to(dt), bias.to(dt) if bias is not None else None,
                               stride=s, padding=padding)
        return apply_act(y.transpose(1, 2), act).to(x.dtype).contiguous()
    if phases is None:
        phases = pack_conv_transpose1d(w, s, padding)
    return _conv_transpose1d_polyphase(x, phases, bias, s, lout, cout, act)


def _conv_transpose1d_polyphase(x, phases, bias, s, lout, cout, act=None):
    """Device-agnostic polyphase evaluation (the HIP path; CPU-testable)."""
    b, L, _ = x.shape
    tmax = -(-lout // s)
    buf = torch.empty(b, tmax * s, cout, dtype=x.dtype, device=x.device)
    view = buf.view(b, tmax, s, cout)
    for r, (wp, pl) in enumerate(phases):
        tr = -(-(lout - r) // s)
        if tr <= 0:
            continue
        o = view[:, :tr, r, :]
        if wp is None:
            o.copy_((bias if bias is not None else torch.zeros(cout, device=x.device)).to(x.dtype).expand_as(o))
            if act is not None:
                o.copy_(apply_act(o.float(), act).to(o.dtype))
            continue
        nt = wp.shape[2]
        pr = tr - L - pl + nt - 1  # makes the conv's output length exactly tr
        if b > 1 and tr != tmax:  # short phase: batch stride != rows * pixel stride -> per sample
            for i in range(b):
                conv1d(x[i:i + 1], wp, bias, padding=(pl, pr), act=act, out=o[i:i + 1])
        else:
            conv1d(x, wp, bias, padding=(pl, pr), act=act, out=o)
    return buf[:, :lout] if tmax * s != lout else buf


def axpby_nhwc(x, z, a, b, out=None, act=None):
    """out = act(a*x + b*z) on NHWC (possibly channel-slice) views; in place
    allowed; ``z`` may be None (then out = act(a*x))."""
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if use_hip(x):
        from . import hip_ops

        if x.dim() == 3:  # token layout [B, T, C] -> [B, 1, T, C] views
            hip_ops.axpby_nhwc(x.unsqueeze(1), z.unsqueeze(1) if z is not None else None, a, b, out.unsqueeze(1), act)
            return out
        return hip_ops.axpby_nhwc(x, z, a, b, out, act)
    y = a * x.to(_cdt(x))
    if z is not None:
        y = y + b * z.to(_cdt(x))
    out.copy_(apply_act(y, act).to(out.dtype))
    return out


def act(x, kind, out=None):
    """Standalone pointwise activation on an NHWC view."""
    return axpby_nhwc(x, None, 1.0, 0.0, out, kind)


def axpby(x, y, a, b):
    """a*x + b*y."""
    if use_hip(x):
        from . import hip_ops

        return hip_ops.axpby(x, y, a, b)
    return (a * x.to(_cdt(x)) + b * y.to(_cdt(x))).to(x.dtype)


# ----------------------------------------------------------------------------
# Normalisation
# ----------------------------------------------------------------------------
def _ref_group_norm(x, gamma, beta, groups, eps, silu):
    dt = _cdt(x)
    c = x.shape[-1]
    xn = x.to(dt).movedim(-1, 1)  # channels-last view [B, C, ...]
    if gamma.dim() == 2:  # per-sample affine [B, C] (scale-shift time conditioning)
        y = F.group_norm(xn, groups, None, None, eps)
        shp = (gamma.shape[0], c) + (1,) * (xn.dim() - 2)
        y = y * gamma.to(dt).view(shp) + beta.to(dt).view(shp)
    else:
        y = F.group_norm(xn, groups, gamma.to(dt), beta.to(dt), eps)
    if silu == "gelu":
        y = F.gelu(y)
    elif silu:
        y = F.silu(y)
    return y.movedim(1, -1).to(x.dtype).contiguous()


def group_norm(x, gamma, beta, groups=32, eps=1e-5, silu=False):
    """GroupNorm over a channels-last tensor [B, ..., C] (+ optional fused
    activation: ``silu=True`` SiLU, ``silu="gelu"`` GELU).  ``gamma``/``beta``
    are [C], or [B, C] (rows may be strided views) for a per-sample affine
    (AdaGroupNorm / scale-shift time conditioning)."""
    if use_hip(x):
        from . import hip_ops

        return hip_ops.group_norm(x, gamma, beta, groups, eps, silu)
    return _ref_group_norm(x, gamma, beta, groups, eps, silu)


def group_norm_cat(a, b, gamma, beta, groups=32, eps=1e-5, silu=False):
    """GroupNorm of the channel concat [a | b] read in place (HIP path, when
    both carry fused epilogue statistics); None when not possible."""
    if use_hip(a):
        from . import hip_ops

        return hip_ops.group_norm_cat(a, b, gamma, beta, groups, eps, silu)
    return None


def _ref_layer_norm(x, gamma, beta, eps):
    dt = _cdt(x)
    return F.layer_norm(x.to(dt), (x.shape[-1],), gamma.to(dt), beta.to(dt) if beta is not None else None,
                        eps).to(x.dtype)


def layer_norm(x, gamma, beta, eps=1e-5):
    if use_hip(x):
        from . import hip_ops

        return hip_ops.layer_norm(x, gamma, beta, eps)
    return _ref_layer_norm(x, gamma, beta, eps)


# ----------------------------------------------------------------------------
# Attention
# ----------------------------------------------------------------------------
def _ref_attention(q, k, v, scale, causal):
    # [B,S,H,D] -> [B,H,S,D]
    if q.is_cuda:
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                           is_causal=causal, scale=scale)
        return o.transpose(1, 2).contiguous()
    qt, kt, vt = (t.permute(0, 2, 1, 3).float() for t in (q, k, v))
    s = (qt @ kt.transpose(-1, -2)) * scale
    if causal:
        sq, sk = s.shape[-2], s.shape[-1]
        mask = torch.ones(sq, sk, dtype=torch.bool, device=s.device).triu(1 + sk - sq)
        s = s.masked_fill(mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = p @ vt
    return o.permute(0, 2, 1, 3).to(q.dtype).contiguous()


def _ref_attention_bias(q, k, v, scale, causal=False, bias=None, kv_lens=None):
    """softmax(q k^T * scale + bias) v over each sample's first ``kv_lens[b]``
    keys, in fp32.  Key j of query i is visible iff j < min(kv_lens[b], Skv) and,
    if ``causal``, j <= i + (Skv - Sq) (aligned against the tensor's Skv:
    padding-mask semantics).  A query row with no visible key (or whose visible
    bias entries are all -inf) gives zeros."""
    B, Sq, H, _ = q.shape
    Skv = k.shape[1]
    qt, kt, vt = (t.permute(0, 2, 1, 3).float() for t in (q, k, v))
    s = (qt @ kt.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.float().expand(B, H, Sq, Skv)
    if kv_lens is not None:
        hidden = torch.arange(Skv, device=s.device)[None, :] >= kv_lens.reshape(B, 1).to(torch.long)
        s = s.masked_fill(hidden[:, None, None, :], float("-inf"))
    if causal:
        mask = torch.ones(Sq, Skv, dtype=torch.bool, device=s.device).triu(1 + Skv - Sq)
        s = s.masked_fill(mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))  # all -inf row: exp(-inf) = 0
    l = p.sum(-1, keepdim=True)
    o = (p @ vt) / torch.where(l > 0, l, torch.ones_like(l))
    return o.permute(0, 2, 1, 3).to(q.dtype).contiguous()


def attention(q, k, v, scale=None, causal=False, kv_len=None, *, bias=None, kv_lens=None):
    """softmax(q k^T * scale) v for [B, S, H, D] views; returns [B, Sq, H, D].
    ``kv_len`` (int32 device tensor [1]): only the first kv_len keys are used;
    read on the device by the HIP kernel (hipGraph-capturable decode step).

    ``bias`` (fp32, broadcastable to [B, H, Sq, Skv]) is added to the scaled
    scores, unscaled; entries may be -inf.  ``kv_lens`` (int32 [B]) gives every
    sample its own key count: a key-padding mask, read on the device.  Unlike
    ``kv_len`` it does not move the causal diagonal, and a query row left with
    no visible key returns zeros.  ``kv_len`` and ``kv_lens`` exclude each other."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if bias is not None or kv_lens is not None:
        if kv_len is not None:
            raise ValueError("attention: kv_len (KV-cache fill level) and kv_lens (per-sample key padding) "
                             "cannot be combined")
        if use_hip(q):
            from . import hip_ops

            return hip_ops.attention_bias(q, k, v, scale, causal, bias, kv_lens)
        return _ref_attention_bias(q, k, v, scale, causal, bias, kv_lens)
    if use_hip(q):
        from . import hip_ops

        return hip_ops.attention(q, k, v, scale, causal, kv_len)
    if kv_len is not None:
        n = int(kv_len.reshape(-1)[0].item())
        k, v = k[:, :n], v[:, :n]
    return _ref_attention(q, k, v, scale, causal)


# ----------------------------------------------------------------------------
# KV-cached decode: one token (or a few rows) per step
# ----------------------------------------------------------------------------
def _ref_rms_norm(x, gamma, eps):
    """fp32 RMSNorm of the last dim (models/llama.py RMSNorm), not rounded"""
    xf = x.float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()


def _ref_decode_norm(x2, ln, rms, what):
    if ln is not None and rms is not None:
        raise ValueError(f"{what}: ln= and rms= exclude each other")
    if ln is not None:
        return _ref_layer_norm(x2, ln[0], ln[1], ln[2])
    if rms is not None:
        return _ref_rms_norm(x2, rms[0], rms[1]).to(_cdt(x2))
    return x2


def gemv(x, w, bias=None, *, act=None, residual=None, ln=None, rms=None, out=None):
    """y[..., N] = act(norm?(x)[..., K] @ w[N, K]^T + bias) + residual for the
    handful of rows of a decode step; ``ln = (gamma, beta, eps)`` LayerNorms the
    rows first, ``rms = (gamma, eps)`` RMSNorms them (one of the two at most).
    Defined as ``gemm(layer_norm(x, *ln), w, bias, residual=, act=)``, resp.
    ``gemm(x.float() * rsqrt(mean(x.float()**2, -1) + eps) * gamma.float(), ...)``,
    which is what runs on the CPU and in reference mode.  On the HIP path up to 8
    rows go to the weight-streaming GEMV kernel (the norm in its prologue, the
    normalised rows never rounded); more rows, K not a multiple of 8 or a GEGLU
    activation run layer_norm / a torch RMSNorm + gemm.
    ``out``: optional [rows, N] view (contiguous last dim) to write into."""
    if ln is not None and rms is not None:
        raise ValueError("gemv: ln= and rms= exclude each other")
    lead = x.shape[:-1]
    k = x.shape[-1]
    x2 = x.reshape(-1, k)
    if use_hip(x):
        from . import hip_ops

        y = hip_ops.gemv(x2, w, bias, act, residual, ln, out, rms)
    else:
        y = _ref_gemm(_ref_decode_norm(x2, ln, rms, "gemv"), w, bias, residual, act).to(x.dtype)
        if out is not None:
            out.copy_(y)
            y = out
    return y.view(*lead, y.shape[-1]) if out is None else y


def gemv_glu(x, w_gate, w_up, *, act="silu", rms=None, ln=None, out=None):
    """Gated two-matrix projection of a decode step (SwiGLU with ``act="silu"``):
    y[..., N] = act(x' @ w_gate[N, K]^T) * (x' @ w_up[N, K]^T), x' = x after the
    optional ``ln`` / ``rms`` norm of ``gemv``.  The two weights stay separate
    tensors (no interleaved or concatenated copy is made).  Defined as
    ``apply_act(_ref_gemm(x', w_gate), act) * _ref_gemm(x', w_up)`` in the input
    dtype (CPU / reference mode).  HIP: up to 8 rows run one launch of the GEMV
    kernel's gated form, a wave streaming the gate row and the up row of each of
    its columns; outside its limits, two ``gemm`` calls and a multiply.  There is
    no bias and no residual."""
    if ln is not None and rms is not None:
        raise ValueError("gemv_glu: ln= and rms= exclude each other")
    if act == "geglu":
        raise ValueError("gemv_glu: act is the gate's pointwise activation, not 'geglu'")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if use_hip(x):
        from . import hip_ops

        y = hip_ops.gemv_glu(x2, w_gate, w_up, act, rms, ln, out)
    else:
        xn = _ref_decode_norm(x2, ln, rms, "gemv_glu")
        y = (_ref_gemm(xn, w_gate, None, None, act) * _ref_gemm(xn, w_up, None, None, None)).to(x.dtype)
        if out is not None:
            out.copy_(y)
            y = out
    return y.view(*lead, y.shape[-1]) if out is None else y


def _ref_rope(x, cos, sin):
    """rotate-half RoPE in fp32: x [..., D], cos / sin broadcastable to [..., D / 2]"""
    h = x.shape[-1] // 2
    xf = x.float()
    a, b = xf[..., :h], xf[..., h:]
    return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)


def decode_attention(q, k_cache, v_cache, scale, kv_len, *, k_new=None, v_new=None, pos=None, rope=None,
                     rel_bias=None):
    """One query per (b, h) over the first ``kv_len`` keys of a [B, S, Hkv, D] KV
    cache; returns [B, 1, H, D].  ``kv_len``: int32 [1] tensor on q's device,
    clamped to [0, S] (0 gives zeros); on the HIP path the kernel reads it, so
    the call is hipGraph-capturable.  With ``k_new`` / ``v_new`` ([B, 1, Hkv, D]
    views, e.g. slices of the QKV projection) the new token's key and value are
    first written into the caches at index kv_len - 1.

    Grouped heads: ``Hkv`` divides ``H``; query head h reads K/V head
    h // (H // Hkv).  ``rope = (cos, sin)``: fp32 [P, D / 2] tables on the device
    (P >= S), row kv_len - 1: the query and the new key are rotated (rotate-half
    form, fp32) before use; the rotated key, rounded to the cache dtype, is what
    is stored and scored, so the caches hold post-RoPE keys.  ``v_new`` is not
    touched; without ``k_new`` only the query is rotated.

    ``rel_bias``: contiguous fp32 [H, P] table on q's device, P >= S, finite
    where it is read: key j of head h scores ``q . k_j * scale +
    rel_bias[h, kv_len - 1 - j]``, a bias indexed by the key's distance to the
    query's own position kv_len - 1 (T5's causal relative-position bias for the
    last query row, ALiBi).  The appended key gets ``rel_bias[h, 0]``; entries at
    distances >= kv_len are never read.  Independent of ``rope`` and of grouped
    heads.

    Definition (CPU / reference): the rotation, that write, the K/V heads
    expanded to the query heads, then ``_ref_attention`` over the first kv_len
    keys (with ``rel_bias``: the same softmax with the bias added to the scaled
    scores).  HIP: the split-KV decode kernel with all of it fused in for D in
    {32, 64, 80, 128} (80 without ``rope``); other head dims do the same steps in
    torch around ``attention(kv_len=)``, resp. ``attention(bias=, kv_lens=)`` with
    the bias row gathered on the device (``pos``: optional long [1] device tensor
    holding kv_len - 1 for that index_copy_, so a caller that has it spares the
    fallback deriving it)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or kv_len.device != q.device:
        raise TypeError("decode_attention: kv_len must be an int32 tensor on the device of q")
    if q.dim() != 4 or q.shape[1] != 1:
        raise ValueError(f"decode_attention: q must be [B, 1, H, D], got {tuple(q.shape)}")
    B, _, H, D = q.shape
    if (k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[0] != B or k_cache.shape[3] != D
            or k_cache.shape[2] < 1 or H % k_cache.shape[2] != 0):
        raise ValueError(f"decode_attention: caches {tuple(k_cache.shape)} / {tuple(v_cache.shape)} do not match "
                         f"q {tuple(q.shape)}")
    Hkv = k_cache.shape[2]
    if (k_new is None) != (v_new is None):
        raise ValueError("decode_attention: k_new and v_new come together")
    if k_new is not None and (k_new.shape != (B, 1, Hkv, D) or v_new.shape != (B, 1, Hkv, D)):
        raise ValueError(f"decode_attention: k_new / v_new {tuple(k_new.shape)} / {tuple(v_new.shape)} must be "
                         f"{(B, 1, Hkv, D)}")
    if rope is not None and (D % 2 or len(rope) != 2):
        raise ValueError("decode_attention: rope = (cos, sin) needs an even head dim")
    if rel_bias is not None and (not isinstance(rel_bias, torch.Tensor) or rel_bias.dtype != torch.float32
                                 or rel_bias.dim() != 2 or rel_bias.shape[0] != H
                                 or rel_bias.shape[1] < k_cache.shape[1] or not rel_bias.is_contiguous()
                                 or rel_bias.device != q.device):
        raise ValueError(f"decode_attention: rel_bias must be a contiguous fp32 [{H}, P >= {k_cache.shape[1]}] "
                         "tensor on the device of q")
    if use_hip(q):
        from . import hip_ops

        return hip_ops.decode_attention(q, k_cache, v_cache, scale, kv_len, k_new, v_new, pos, rope, rel_bias)
    n = min(max(int(kv_len.reshape(-1)[0].item()), 0), k_cache.shape[1])
    if n == 0:
        return torch.zeros_like(q)
    if rope is not None:
        cos, sin = rope[0][n - 1].float(), rope[1][n - 1].float()
        q = _ref_rope(q, cos, sin).to(q.dtype)
        if k_new is not None:
            k_new = _ref_rope(k_new, cos, sin)
    if k_new is not None:
        k_cache[:, n - 1] = k_new[:, 0].to(k_cache.dtype)
        v_cache[:, n - 1] = v_new[:, 0].to(v_cache.dtype)
    k, v = k_cache[:, :n], v_cache[:, :n]
    if Hkv != H:
        k, v = (t[:, :, :, None].expand(B, n, Hkv, H // Hkv, D).reshape(B, n, H, D) for t in (k, v))
    if rel_bias is not None:  # key j at distance n - 1 - j from the query
        bias = rel_bias[:, torch.arange(n - 1, -1, -1, device=q.device)]
        return _ref_attention_bias(q, k, v, scale, False, bias[:, None])
    return _ref_attention(q, k, v, scale, False)


# ----------------------------------------------------------------------------
# Image preprocessing
# ----------------------------------------------------------------------------
def canny(gray: torch.Tensor, low: float = 100.0, high: float = 200.0) -> torch.Tensor:
    """Canny edges of a uint8 [H, W] image (0/255), cv2 semantics."""
    if use_hip(gray):
        from . import hip_ops

        return hip_ops.canny(gray, low, high)
    from ..controlnet.preprocess import canny_np

    return torch.from_numpy(canny_np(gray.cpu().numpy(), float(low), float(high))).to(gray.device)


# ----------------------------------------------------------------------------
# Elementwise
# ----------------------------------------------------------------------------
def dup2(x):
    """[x; x] along the batch dim (one kernel on the HIP path)."""
    if use_hip(x):
        from . import hip_ops

        y = hip_ops.dup2(x)
        st = getattr(x, "_csk_gn", None)
        if st is not None:  # epilogue GN partials are batch-major [B*P/seg][C][2]: duplicate them too
            y._csk_gn = (torch.cat([st[0], st[0]]), st[1])
        return y
    return torch.cat([x, x], 0)


def silu(x):
    if use_hip(x):
        from . import hip_ops

        return hip_ops.silu(x)
    return F.silu(x.to(_cdt(x))).to(x.dtype)


def add(x, y):
    if use_hip(x):
        from . import hip_ops

        return hip_ops.add(x, y)
    return (x.to(_cdt(x)) + y.to(_cdt(x))).to(x.dtype)


# ----------------------------------------------------------------------------
# Sampler step (CFG combine + x0 + linear update) and VAE post-process
# ----------------------------------------------------------------------------
def _ref_sched_step(e, x, prev_x0, c, guidance, noise):
    ef = e.float()
    if guidance is not None:
        e_u, e_c = ef.chunk(2)
        ef = e_u + guidance * (e_c - e_u)
    x0 = c.p * x + c.q * ef
    out = c.A * x + c.B * x0
    if c.C != 0.0 and prev_x0 is not None:
        out = out + c.C * prev_x0
    if c.D != 0.0 and noise is not None:
        out = out + c.D * noise
    return out, x0


def sched_step(e, x, sched, coeffs, guidance=None, noise=None):
    """Fused CFG + sampler update.  Updates ``sched`` state
    (prev_x0, step_index) and returns the new fp32 latents."""
    prev = sched.prev_x0
    if use_hip(x):
        from . import hip_ops

        out, x0 = hip_ops.sched_step(e, x, prev, coeffs, guidance, noise)
    else:
        out, x0 = _ref_sched_step(e, x, prev, coeffs, guidance, noise)
    sched.prev_x0 = x0
    sched.step_index += 1
    return out


def vae_postprocess(img):
    """NHWC [-1, 1] -> uint8 NHWC (x/2+0.5).clamp(0,1)*255 rounded (K15)."""
    if use_hip(img):
        from . import hip_ops

        return hip_ops.vae_postprocess(img)
    return ((img.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)
