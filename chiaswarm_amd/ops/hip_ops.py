"""ctypes bindings of the gfx950 kernels in libcsk.so.

Every function allocates its output with the torch caching allocator and
launches on torch's current stream (graph-capture safe: no host syncs, no
hipMalloc).  Shape/stride preconditions are checked on the host BEFORE launch
so a bad call raises here instead of faulting the GPU.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib, tuning
from ._lib import c_float, c_int, c_int64, c_void_p, sig

ACT = {None: 0, "none": 0, "gelu": 1, "silu": 2, "geglu": 3, "quick_gelu": 4}

sig("csk_gemm", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, c_void_p, c_void_p)
sig("csk_conv2d", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p)
sig("csk_gemm_ln", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p,
    c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p)
sig("csk_conv2d_ex", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p)
sig("csk_group_norm_part", c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
    c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p)
sig("csk_group_norm_part2", c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
    c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p)


# ---------------------------------------------------------------------------
# GroupNorm statistics fused into producer epilogues
# ---------------------------------------------------------------------------
GN_FINE = 0  # mirrors the library's g_gn_fine (set_gn_fine)


def set_gn_fine(v: int):
    global GN_FINE
    GN_FINE = int(v)
    _lib.call("csk_set_gn_fine", GN_FINE)


GN_TARGET_WG = 512  # GroupNorm apply/stats workgroups per call (rows per chunk follow); 512: -0.05 ms/step vs 1024 (tools/abstep.py gnwgN, profiles/unet_step_ab_gnwg_r3e.txt)
SPLITK_GN_SEG = 64  # gemm_common.h SPLITK_GN_SEG: segment rows of the split-K reduce's GN statistics
SPLITK_GN = True  # split-K producers emit GN statistics from their reduce (tools/abstep.py arms skgn0 / skgn1)


def _gn_seg(tile, split, rows_per_b, M, code, N=8):
    """Rows per fused-GN statistics segment (fine: the epilogue's column pass
    splits each BM-row tile into 256/BN segments of BM*BN/256 rows; else one
    segment per tile; split-K: the reduce kernel's SPLITK_GN_SEG rows), or 0."""
    bm, bn = tuning.TILES.get(tile, (0, 0))
    if code == 3 or bm == 0 or rows_per_b <= 0:
        return 0
    if split > 1:  # (split < 0, the in-kernel fixup, writes the tile's own segments)
        if not SPLITK_GN:
            return 0
        s = SPLITK_GN_SEG
        return s if rows_per_b % s == 0 and M % s == 0 and N % 8 == 0 else 0
    if rows_per_b % bm or M % bm:
        return 0
    seg = bm * bn // 256 if GN_FINE else bm
    band = bm // tuning.EPI_WM.get(tile, 2) if (bm > 128 or bn == 160) else bm  # epilogue row band (epi_passes)
    return min(seg, band)


def _ws(split, M, N, device):
    """fp32 split-K workspace: [split][M][N] for the reduce kernel; split < 0
    (in-kernel fixup, gemm_common.h splitk_fixup) stores whole padded tiles, at
    most (M + 255) x (N + 255) outputs per split for every tile geometry"""
    if split > 1:
        return torch.empty(split * M * N, dtype=torch.float32, device=device)
    if split < 0:
        return torch.empty(-split * (M + 255) * (N + 255), dtype=torch.float32, device=device)
    return None


def _gn_part(M, N, seg, device):
    return torch.empty((M // seg) * N * 2, dtype=torch.float32, device=device)
sig("csk_axpby", c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p)
ACT.update({"lrelu": 5, "lrelu0.1": 6, "tanh": 7, "relu": 8, "lrelu0.01": 9, "elu": 10, "gelu_tanh": 11})
sig("csk_group_norm", c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
    c_int, c_int, c_float, c_int, c_int, c_void_p)
sig("csk_layer_norm", c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p)
ATTN_VARIANT = int(os.environ.get("CSK_ATTN", "0"))  # 0 auto, 1 plain, 2 pipelined (D <= 64)
sig("csk_attention", c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int,
    c_int, c_float, c_int, c_int, c_void_p, c_void_p)
sig("csk_silu", c_void_p, c_void_p, c_int64, c_void_p)
sig("csk_canny", c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p)
sig("csk_add", c_void_p, c_void_p, c_void_p, c_int64, c_void_p)
sig("csk_sched_step", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
    c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_int, c_void_p)
sig("csk_vae_post", c_void_p, c_void_p, c_int64, c_void_p)
sig("csk_loop_prologue", c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p)
sig("csk_sched_loop", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64,
    c_int, c_void_p)
LOOP_COEF_STRIDE = 12  # elementwise.hip: {p, q, A, B, C, D, s_next, g, g2, -, -, -} per step
sig("csk_pad_channels", c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p)
sig("csk_set_gn_prologue_max", c_int)
sig("csk_debug_selftest", c_int, c_void_p)  # CSK_DEBUG builds: one deliberate record (tests)
sig("csk_set_gn_lds", c_int)
sig("csk_set_sw_odd", c_int)
sig("csk_set_epi_band", c_int)
sig("csk_set_epi_nt", c_int)
sig("csk_set_skr_unroll", c_int)
sig("csk_set_short_kv_variant", c_int)
sig("csk_set_short_kv_rows", c_int)
sig("csk_set_attn32", c_int)
sig("csk_xattn_block", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
    c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p)
sig("csk_attention_fa", c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int,
    c_int, c_float, c_int, c_void_p)
sig("csk_set_attn_fa", c_int)
sig("csk_attn_fa_ok", c_int, c_int, c_int, c_int, c_int, c_int, c_int)
sig("csk_attention_split", c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int,
    c_int, c_float, c_int, c_void_p, c_void_p, c_void_p)
sig("csk_dup2", c_void_p, c_void_p, c_int64, c_void_p)
sig("csk_row_bcast", c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p)
sig("csk_set_ln_in_kernel", c_int)
sig("csk_set_gn_finalize_wg", c_int)
sig("csk_set_gn_cb", c_int)
sig("csk_set_gn_cb_mult", c_int)
sig("csk_set_gn_cb_small", c_int)
sig("csk_set_gn_fine", c_int)
sig("csk_timestep_embedding", c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p)


def timestep_embedding(t, batch, dim, flip_sin_to_cos=True, shift=0.0, max_period=10000.0):
    """bf16 [batch, dim] sinusoidal embedding of fp32 timesteps t ([1] broadcast or [batch])."""
    t = t.reshape(-1)
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    if t.numel() not in (1, batch):
        raise ValueError(f"timestep_embedding: {t.numel()} timesteps for batch {batch}")
    y = torch.empty((batch, dim), dtype=torch.bfloat16, device=t.device)
    _lib.call("csk_timestep_embedding", _p(y), _p(t), 0 if t.numel() == 1 else 1, batch, dim,
              int(bool(flip_sin_to_cos)), float(shift), float(max_period), _s())
    return y


def _bf16(t, name):
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name}: HIP kernels take bfloat16, got {t.dtype}")


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return _lib.stream_ptr()


def _round8(n):
    return (n + 7) // 8 * 8


def pad_last(x: torch.Tensor, n: int) -> torch.Tensor:
    """Zero-pad the last (contiguous) dim of a bf16 tensor to n."""
    c = x.shape[-1]
    if c == n:
        return x
    x = x.contiguous()
    y = torch.empty(x.shape[:-1] + (n,), dtype=x.dtype, device=x.device)
    rows = x.numel() // c
    _lib.call("csk_pad_channels", _p(y), _p(x), rows, c, n, _s())
    return y


# ---------------------------------------------------------------------------
def gemm(a2, w, bias=None, residual=None, act=None, out=None, gn_rows=0, ln=None, row_stats=False):
    """``gn_rows`` > 0: also produce GroupNorm statistics of the output for a
    consumer GN (rows per sample = gn_rows), attached as ``out._csk_gn``.

    ``row_stats``: also produce per-row (mean, M2) partials of the output for a
    consumer's fused LayerNorm, attached as ``out._csk_rows = (part, nparts, pcols)``.
    ``ln = (rows, colsum, eps)``: this GEMM's input rows are LayerNorm'd on the
    fly — ``w``/``bias`` are the gamma/beta-folded weights (``fold_layer_norm``)
    and ``rows`` the producer's ``_csk_rows``."""
    _bf16(a2, "gemm.a")
    _bf16(w, "gemm.w")
    M, K = a2.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm: K mismatch {a2.shape} x {w.shape}")
    if a2.stride(1) != 1 or a2.stride(0) % 8 != 0 or (a2.data_ptr() % 16):
        a2 = a2.contiguous()
    if w.stride(1) != 1 or w.stride(0) % 8 != 0:
        w = w.contiguous()
    if K % 8 != 0:
        kp = _round8(K)
        a2 = pad_last(a2, kp)
        w = pad_last(w, kp)
        K = kp
    code = ACT[act]
    n_out = N // 2 if code == 3 else N
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.bfloat16, device=a2.device)
    if residual is not None:
        residual = residual.reshape(M, n_out)
        _bf16(residual, "gemm.residual")
        if not residual.is_contiguous():
            residual = residual.contiguous()
    if bias is not None:
        _bf16(bias, "gemm.bias")
    lda, ldb = a2.stride(0), w.stride(0)

    def run(tile, split, part=None):
        ws = _ws(split, M, N, a2.device)
        _lib.call("csk_gemm", _p(out), _p(a2), _p(w), _p(bias), None, _p(residual),
                  M, N, K, lda, ldb, n_out, n_out, 1, code, 1.0, _p(part), tile, split, _p(ws), _s())

    tile, split = tuning.choose(f"g:{M}:{N}:{K}:{code}", M, N, K, run)
    if split < 0 and tile not in tuning.GLDS:
        split = 1  # the in-kernel fixup exists in the LDS-DMA tiles only
    if ln is not None or row_stats:
        if split > 1:  # the split-K reduce has no LN / row-statistics epilogue
            tile, split = (19 if N <= 1280 else 20), 1
        # mirror the library's own tile substitutions: the row-statistics slabs
        # (and the buffer sized for them below) follow the tile that actually runs
        if tile in (25, 26, 31, 32, 33, 34):  # 160-column and 8-wave tiles: no LN / row statistics -> tile 11
            tile = 11
        elif tile == 36:  # 64x160 -> 64x128 (gemm_glds.hip csk_gemm_glds_launch)
            tile = 13
        if ln is None and code == 3:
            row_stats = False
    seg = _gn_seg(tile, split, gn_rows, M, code, N) if gn_rows and out.is_contiguous() else 0
    part = _gn_part(M, N, seg, a2.device) if seg else None
    if ln is None and not row_stats:
        run(tile, split, part)
    else:
        bn = tuning.TILES[tile][1]
        rp = torch.empty(-(-N // bn) * M * 2, dtype=torch.float32, device=a2.device) if row_stats else None
        lp = lc = rowbuf = None
        nparts = pcols = 0
        eps = 0.0
        if ln is not None:
            (lp, nparts, pcols), lc, eps = ln
            if K % 8 or nparts * pcols < K or lp.numel() < nparts * M * 2:
                raise ValueError("gemm: fused LayerNorm statistics do not match the input")
            rowbuf = torch.empty(M * 2, dtype=torch.float32, device=a2.device)
        _lib.call("csk_gemm_ln", _p(out), _p(a2), _p(w), _p(bias), None, _p(residual),
                  M, N, K, lda, ldb, n_out, n_out, 1, code, 1.0, _p(part), _p(lp), _p(lc), nparts, pcols,
                  float(eps), _p(rowbuf), _p(rp), tile, 1, None, _s())
        if rp is not None:
            out._csk_rows = (rp, -(-N // bn), bn)
    if part is not None:
        out._csk_gn = (part, seg)
    return out


# Cross-attention query projection with the attention in the GEMM epilogue
# (gemm_common.h gemm_attn_epilogue): O = softmax(q K^T * scale) V straight from
# the Q-projection accumulators, one head per 128x64 tile.
sig("csk_gemm_ln_attn", c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
    c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p)
QATTN = os.environ.get("CSK_QATTN", "1") == "1"
# below this many 128x64 tiles the one-head-per-tile grid under-fills the chip
# and the unfused query GEMM + short-KV attention win (CFG batch 2 of SD2.1:
# 80 / 160 tiles, +0.01 ms/step; batch 8: 320 / 640 tiles, -0.09 ms/step,
# profiles/unet_step_ab_qattn_r6s.txt)
QATTN_MIN_TILES = int(os.environ.get("CSK_QATTN_MIN_TILES", "256"))
QATTN_STATS = [0]  # calls (tests assert the fused path ran)


def qattn_ok(x, kv, rows_per_b) -> bool:
    """Shapes the attention-epilogue GEMM takes: head dim 64 (heads = C / 64),
    <= 80 context tokens, 128-row tiles inside one sample."""
    C = x.shape[-1]
    M = x.numel() // C
    return (QATTN and kv is not None and kv.dim() == 5 and kv.shape[2] == 2 and kv.shape[4] == 64
            and kv.shape[3] * 64 == C and 1 <= kv.shape[1] <= 80 and C % 64 == 0 and rows_per_b % 128 == 0
            and M % rows_per_b == 0 and kv.shape[0] >= M // rows_per_b
            and (M // 128) * (C // 64) >= QATTN_MIN_TILES)


def gemm_attn(a2, w, bias, kv, scale, rows_per_b, ln=None, tile=None):
    """Attention output O [M, C] of the cross-attention whose query projection
    is ``a2 @ w^T + bias`` (``ln = (rows, colsum, eps)``: LayerNorm folded as in
    ``gemm``), over the per-request ``kv`` [Bc, Skv, 2, H, 64]."""
    _bf16(a2, "gemm_attn.a")
    _bf16(w, "gemm_attn.w")
    _bf16(kv, "gemm_attn.kv")
    M, K = a2.shape
    N = w.shape[0]
    if w.shape[1] != K or K % 8:
        raise ValueError(f"gemm_attn: K mismatch {a2.shape} x {w.shape}")
    if a2.stride(1) != 1 or a2.stride(0) % 8 != 0 or (a2.data_ptr() % 16):
        a2 = a2.contiguous()
    w = w.contiguous()
    kv = kv.contiguous()
    if bias is not None:
        _bf16(bias, "gemm_attn.bias")
        bias = bias.contiguous()
    # 128x64 row-layout tile: 3-stage (12) for the long-K C = 1280 projections,
    # 2-stage (19) otherwise (18.3 vs 19.1 us at K = 1280, 21.7 vs 18.9 at K = 640;
    # profiles/qattnbench_r7a.txt)
    if tile is None:
        tile = 12 if K >= 1280 else 19
    elif tile not in (12, 19):
        raise ValueError("gemm_attn: tile 12 or 19")
    out = torch.empty((M, N), dtype=torch.bfloat16, device=a2.device)
    lp = lc = rowbuf = None
    nparts = pcols = 0
    eps = 0.0
    if ln is not None:
        (lp, nparts, pcols), lc, eps = ln
        if nparts * pcols < K or lp.numel() < nparts * M * 2:
            raise ValueError("gemm_attn: fused LayerNorm statistics do not match the input")
        rowbuf = torch.empty(M * 2, dtype=torch.float32, device=a2.device)
    QATTN_STATS[0] += 1
    _lib.call("csk_gemm_ln_attn", _p(out), _p(a2), _p(w), _p(bias), M, N, K, a2.stride(0), w.stride(0), N,
              int(rows_per_b), _p(lp), _p(lc), nparts, pcols, float(eps), _p(rowbuf), _p(kv), int(kv.shape[0]),
              int(kv.shape[1]), float(scale), tile, _s())
    return out


def _pix_stride(t):
    """Pixel stride of an NHWC tensor / channel-slice view (None if not NHWC-strided)."""
    B, H, W, C = t.shape
    s = t.stride()
    if s[3] != 1:
        return None
    ps = s[2]
    if (W > 1 and s[2] != ps) or (H > 1 and s[1] != W * ps) or (B > 1 and s[0] != H * W * ps):
        return None
    return ps


# Persistent halo-tile conv for 3x3 / stride-1 / Cout = 16 / 32 / 64 and < 16
# (csrc/kernels/conv_tile.hip: the Real-ESRGAN dense-block convs, its x2
# up-convs and RGB conv_last); CSK_CONV_TILE=0 keeps the implicit GEMM
sig("csk_conv_tile_ok2", c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int)
sig("csk_conv_tile2", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_void_p)
CONV_TILE = os.environ.get("CSK_CONV_TILE", "1") == "1"
CONV_TILE64 = os.environ.get("CSK_CONV_TILE64", "1") == "1"  # the Cout = 64 instance: 1.2x faster than the GEMM (profiles/conv_tile64_r5.txt)
# Cout <= 16 (16-wide instance; e.g. the x4 upscaler's 64 -> 3 conv_last at 2048^2) on
# maps of at least this many output pixels (below it the grid is a fraction of the chip)
CONV_TILE_NARROW_MIN_PX = int(os.environ.get("CSK_CONV_TILE_NARROW_MIN_PX", str(1 << 18)))
CONV_TILE_STATS = [0]  # calls (tests assert the kernel ran)

# Split-K conv whose reduce also applies the GroupNorm (+ SiLU) that follows it
# (gemm.hip splitk_reduce_gn_apply_kernel; conv2d's ``norm`` argument).
# CSK_SKGN_FUSED=0 / set_skgn_fused(False): the split-K reduce and the
# GroupNorm apply stay two kernels.
sig("csk_set_skgn_fused", c_int)
sig("csk_set_skgn_min_wg", c_int)
sig("csk_get_skgn_min_wg")
sig("csk_get_skr_unroll")
sig("csk_splitk_gn_fused_ok", c_int, c_int, c_int, c_int)
sig("csk_conv2d_gn", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int,
    c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_int, c_int, c_void_p)
# conv with extra K segments (a ResNet's 1x1 shortcut folded into its conv2's K loop)
sig("csk_conv2d_ex2", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int,
    c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p)
sig("csk_conv2d_gn2", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int,
    c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
    c_int, c_void_p)
SC_FUSE_STATS = [0]  # conv2d(extra=...) launches (tests assert the fused path ran)
# tiles that walk extra K segments: the LDS-DMA rings (gemm_glds.hip, gemm8p.hip gemm8r_kernel)
XS_TILES = tuning.GLDS | {33, 34}
# (B, H, W, Cin, Cout, segment channels) the fused conv measured slower at than
# conv2 + the shortcut GEMMs it replaces (tools/convbench.py --shortcut): kept unfused
SC_FUSE_OFF = set()


def conv_extra_ok(x, wp, extra, stride=1, padding=1, up2x=False, dilation=1) -> bool:
    """``conv2d(extra=...)`` takes this call on the HIP path: FAST LDS-DMA
    staging (every channel count a multiple of 64), 3x3-style same-size geometry
    (stride 1, no upsample, dilation 1, output size == input size), sources that
    are 16-byte aligned NHWC tensors / channel slices of the output's
    [B, Ho, Wo] with a pixel stride that is a multiple of 8, and a weight pack
    ``fused_weight`` recognises."""
    from . import conv_out_size

    if not extra or len(extra) > 2 or x.dim() != 4 or x.dtype != torch.bfloat16:
        return False
    B, H, W, Cin = x.shape
    Cout, kh, kw, _ = wp.shape
    if stride != 1 or up2x or dilation != 1 or Cin % 64 or conv_out_size(H, W, kh, kw, 1, padding) != (H, W):
        return False
    xs = _pix_stride(x)
    if xs is None or xs % 8 or x.data_ptr() % 16:
        return False
    for a, wa in extra:
        if a.dtype != torch.bfloat16 or a.dim() != 4 or tuple(a.shape[:3]) != (B, H, W) or a.shape[3] % 64:
            return False
        ps = _pix_stride(a)
        if ps is None or ps % 8 or a.data_ptr() % 16 or tuple(wa.shape) != (Cout, a.shape[3]):
            return False
    if (B, H, W, Cin, Cout, tuple(a.shape[3] for a, _ in extra)) in SC_FUSE_OFF:
        return False
    return fused_weight(wp, extra) is not None


def fused_weight(wp, extra):
    """The [Cout, kh*kw*Cin + Ca (+ Cb)] K-contiguous matrix that ``wp`` and the
    segment weights are consecutive column slices of (``ops.pack_conv_extra``),
    or None when they are separate tensors."""
    Cout, kh, kw, Cin = wp.shape
    k0 = kh * kw * Cin
    K = k0 + sum(w.shape[1] for _, w in extra)
    if wp.dtype != torch.bfloat16 or wp.stride() != (K, kw * Cin, Cin, 1) or wp.data_ptr() % 16:
        return None
    off = k0
    for _, w in extra:
        if w.dtype != wp.dtype or w.stride() != (K, 1) or w.data_ptr() != wp.data_ptr() + 2 * off:
            return None
        off += w.shape[1]
    return torch.as_strided(wp, (Cout, K), (K, 1))


SKGN_FUSED = os.environ.get("CSK_SKGN_FUSED", "1") == "1"
# conv2d(norm=...) calls: (norm applied in the reduce, conv + GroupNorm kernels here,
# norm_optional: raw returned and the norm left to its consumer)
SKGN_STATS = [0, 0, 0]
SKGN_SITES = None  # tools: a list here collects (B, Ho, Wo, Cin, Cout, split, keep_raw) of every fused call


def set_skgn_fused(on: bool):
    global SKGN_FUSED
    SKGN_FUSED = bool(on)
    _lib.call("csk_set_skgn_fused", int(SKGN_FUSED))


def set_skgn_min_wg(n: int) -> int:
    """Smallest grid (samples x groups) the fused kernel takes; returns the previous value."""
    old = _lib.call_int("csk_get_skgn_min_wg")
    _lib.call("csk_set_skgn_min_wg", int(n))
    return old


def _eff_split(split, K):
    """The split count the library runs for a requested ``split`` > 1 (gemm.hip
    dispatch: whole 64-wide K steps per split, empty splits dropped)."""
    if split <= 1:
        return split
    kchunk = -(-(-(-K // 64)) // split) * 64
    return -(-K // kchunk)


def _skgn_ok(split, K, M, Cout, rows_per_b, ys, code, gamma, beta, groups, silu, bias, bias2d, b2s, residual, rs,
             out, keep_raw):
    """The fused reduce + GroupNorm apply takes this conv: a split-K plan, no
    activation, shared [C] affine, 8-byte aligned 4-channel vectors everywhere,
    one sample's group within the kernel's register budget."""
    if not SKGN_FUSED or _eff_split(split, K) <= 1 or code != 0 or gamma.dim() != 1 or silu not in (True, False):
        return False
    if gamma.dtype != torch.bfloat16 or beta.dtype != torch.bfloat16 or gamma.numel() != Cout or beta.numel() != Cout:
        return False
    if not (gamma.is_contiguous() and beta.is_contiguous()):
        return False
    for t in (gamma, beta, bias, bias2d, residual, out if keep_raw else None):
        if t is not None and t.data_ptr() % 8:
            return False
    if (keep_raw and ys % 4) or (residual is not None and rs % 4) or (bias2d is not None and b2s % 4):
        return False
    return _lib.call_int("csk_splitk_gn_fused_ok", M, Cout, rows_per_b, int(groups)) > 0


def conv2d(x, wp, bias, stride, padding, residual, up2x, bias2d, act=None, out_scale=1.0, out=None, dilation=1,
           gn_stats=False, residual2=None, res_scale=1.0, out_u8=False, norm=None, norm_optional=False, extra=None):
    """NHWC conv.  ``x``, ``residual`` and ``out`` may be channel-slice views of
    wider NHWC buffers (last dim contiguous): the kernel takes their pixel
    strides, so dense/concat blocks need no copies.  ``residual2`` /
    ``res_scale`` (y = ... * out_scale + res_scale * residual + residual2, ``out``
    may alias ``residual2``) run in the halo-tile kernel's epilogue, elsewhere as
    one extra pass.  ``out_u8``: uint8 image output round(clamp(y, 0, 1) * 255)
    (the halo-tile kernel stores it directly for Cout < 16).
    ``norm = (gamma, beta, groups, eps, silu, keep_raw)``: the GroupNorm (+ SiLU)
    that consumes the output; returns the normalised tensor, or (normalised, raw)
    with ``keep_raw``.  A split-K plan applies it in its reduce kernel
    (SKGN_STATS[0]); anything else is this conv followed by ``group_norm``, or,
    with ``norm_optional`` (and ``keep_raw``), returns (None, raw) and leaves the
    norm to the consumer of the raw tensor (its epilogue statistics attached).
    ``extra = ((a, wa), (b, wb))``: y = conv(x) + a . wa^T (+ b . wb^T) as extra
    K segments of the conv's own K loop (one fp32 accumulation); ``wp`` and the
    segment weights are slices of one ``ops.pack_conv_extra`` matrix and
    ``conv_extra_ok`` holds, anything else is an error."""
    from . import conv_out_size, norm_padding

    if extra is not None:
        if out_u8 or residual2 is not None or res_scale != 1.0:
            raise ValueError("conv2d: extra with out_u8 / residual2 / res_scale")
        if not conv_extra_ok(x, wp, extra, stride, padding, up2x, dilation):
            raise ValueError("conv2d: extra K segments need conv_extra_ok() (64-channel multiples, same-size "
                             "stride-1 conv, aligned NHWC sources, one packed weight)")
    if norm is not None:
        if out_u8 or residual2 is not None or res_scale != 1.0:
            raise ValueError("conv2d: norm with out_u8 / residual2 / res_scale")
        if out is not None and not norm[5]:
            raise ValueError("conv2d: out= with norm is the raw output: it needs keep_raw")
        gn_stats = True  # where the reduce does not apply the norm, its statistics come from the conv

    _bf16(x, "conv.x")
    _bf16(wp, "conv.w")
    B, H, W, Cin = x.shape
    xs = _pix_stride(x)
    if xs is None or xs % 8 != 0 or Cin % 8 != 0 or x.data_ptr() % 16:
        x = x.contiguous()
        xs = Cin
    Cout, kh, kw, Cw = wp.shape
    if Cw != Cin:
        raise ValueError(f"conv2d: Cin mismatch {tuple(x.shape)} vs {tuple(wp.shape)}")
    if Cin % 8 != 0:
        cp = _round8(Cin)
        x = pad_last(x, cp)
        wp = pad_last(wp.contiguous(), cp)
        Cin = xs = cp
    wf, xseg = None, ()
    if extra is not None:
        wf = fused_weight(wp, extra)
        xseg = tuple((a, _pix_stride(a), a.shape[3]) for a, _ in extra)
    else:
        wp = wp.contiguous()
    pt, pl, pb, pr = norm_padding(padding)
    Ho, Wo = conv_out_size(H, W, kh, kw, stride, padding, up2x, dilation)
    if out_u8:
        return _conv2d_u8(x, wp, bias, stride, padding, residual, up2x, bias2d, act, out_scale, out, dilation,
                          residual2, res_scale, Ho, Wo)
    oshape = (B, Ho, Wo, Cout)
    if out is None and (norm is None or norm[5]):
        out = torch.empty(oshape, dtype=torch.bfloat16, device=x.device)
    # norm without keep_raw: the raw tensor is allocated only if the reduce does not apply the norm
    ys = Cout if out is None else _pix_stride(out)
    if out is not None and (out.shape != oshape or ys is None):
        raise ValueError(f"conv2d out {tuple(out.shape)} / strides unsupported")
    rs = 0
    if residual is not None:
        if tuple(residual.shape) != oshape:
            raise ValueError(f"conv2d residual {tuple(residual.shape)} != {oshape}")
        rs = _pix_stride(residual)
        if rs is None:
            residual = residual.contiguous()
            rs = Cout
    b2s = 0
    if bias2d is not None:
        # a column slice of the UNet's one batched time-embedding GEMM: pass its
        # row stride instead of copying it out (one copy kernel per ResNet)
        if bias2d.shape != (B, Cout):
            raise ValueError("conv2d bias2d shape")
        _bf16(bias2d, "conv.bias2d")
        if bias2d.stride(1) != 1 or bias2d.data_ptr() % 16 or bias2d.stride(0) % 8:
            bias2d = bias2d.contiguous()
        b2s = bias2d.stride(0) if B > 1 else Cout
    M, K = B * Ho * Wo, kh * kw * Cin + sum(s[2] for s in xseg)
    code = ACT[act]
    # the segment arguments of the *2 entry points: (a, pixel stride, channels) x 2
    sargs = ()
    if xseg:
        sb = xseg[1] if len(xseg) > 1 else (None, 0, 0)
        sargs = (_p(xseg[0][0]), xseg[0][1], xseg[0][2], _p(sb[0]), sb[1], sb[2])

    def run(tile, split, part=None):
        nonlocal out
        if out is None:  # norm without keep_raw, and the reduce does not apply it (or tuning.choose is timing plans)
            out = torch.empty(oshape, dtype=torch.bfloat16, device=x.device)
        ws = _ws(split, M, Cout, x.device)
        if xseg:
            _lib.call("csk_conv2d_ex2", _p(out), _p(x), _p(wf), _p(bias), _p(bias2d), b2s, _p(residual),
                      B, H, W, Cin, Cout, kh, kw, stride, pt, pl, Ho, Wo, 0, xs, ys, rs, code,
                      float(out_scale), int(dilation), _p(part), tile, split, _p(ws), *sargs, _s())
            return
        _lib.call("csk_conv2d_ex", _p(out), _p(x), _p(wp), _p(bias), _p(bias2d), b2s, _p(residual),
                  B, H, W, Cin, Cout, kh, kw, stride, pt, pl, Ho, Wo, int(bool(up2x)), xs, ys, rs, code,
                  float(out_scale), int(dilation), _p(part), tile, split, _p(ws), _s())

    rs2 = 0
    if residual2 is not None:
        if tuple(residual2.shape) != oshape:
            raise ValueError(f"conv2d residual2 {tuple(residual2.shape)} != {oshape}")
        rs2 = _pix_stride(residual2)
        if rs2 is None:
            residual2 = residual2.contiguous()
            rs2 = Cout
    key = f"c:{B}:{H}:{W}:{Cin}:{Cout}:{kh}:{stride}:{int(bool(up2x))}"
    if kh != kw or dilation != 1:
        key += f":{kw}:{dilation}"
    narrow = Cout < 16
    if xseg:
        # its own entries (K differs); a miss runs the unfused conv's plan
        fkey = key + ":x" + ":".join(str(s[2]) for s in xseg)
        tile, split = tuning.choose_extra(fkey, key, M, Cout, K, run, XS_TILES)
        SC_FUSE_STATS[0] += 1
    elif (CONV_TILE and kh == 3 and kw == 3 and stride == 1 and (pt, pl, pb, pr) == (1, 1, 1, 1) and dilation == 1
            and bias2d is None and not gn_stats
            and code in (0, 2, 5, 6, 8, 9)
            and (Cout == 32 or (Cout == 64 and CONV_TILE64) or (Cout <= 16 and M >= CONV_TILE_NARROW_MIN_PX))
            and (residual is None or (not narrow and rs % 4 == 0 and residual.data_ptr() % 8 == 0))
            and (residual2 is None or (not narrow and rs2 % 4 == 0 and residual2.data_ptr() % 8 == 0))
            and _lib.call_int("csk_conv_tile_ok2", B, Ho, Wo, Cin, Cout, xs, ys, int(bool(up2x))) > 0
            and x.data_ptr() % 16 == 0 and (narrow or out.data_ptr() % 8 == 0) and wp.data_ptr() % 16 == 0):
        # narrow-output 3x3 (the Real-ESRGAN convs): persistent halo-tile kernel
        _lib.call("csk_conv_tile2", _p(out), _p(x), _p(wp), _p(bias), _p(residual), _p(residual2), B, Ho, Wo, Cin,
                  Cout, xs, ys, rs, rs2, code, float(out_scale), float(res_scale), int(bool(up2x)), 0, _s())
        CONV_TILE_STATS[0] += 1
        return out  # never with a norm: it sets gn_stats, which this kernel does not produce
    elif residual2 is not None or res_scale != 1.0:
        # the implicit GEMM's epilogue has one unscaled residual: conv into a
        # temporary, then one combining pass (residual2 is read before out is written)
        y = conv2d(x, wp, bias, stride, padding, None, up2x, bias2d, act, out_scale, None, dilation)
        if residual is not None:
            y = torch.add(y, residual, alpha=res_scale) if res_scale != 1.0 else y + residual
        if residual2 is not None:
            y = y + residual2
        out.copy_(y)
        return out
    else:
        tile, split = tuning.choose(key, M, Cout, K, run)
    if norm is not None:
        gamma, beta, groups, eps, silu, keep_raw = norm
        if ys == Cout and _skgn_ok(split, K, M, Cout, Ho * Wo, ys, code, gamma, beta, groups, silu, bias, bias2d, b2s,
                                   residual, rs, out, keep_raw):
            yn = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
            ws = _ws(split, M, Cout, x.device)
            _lib.call("csk_conv2d_gn2" if xseg else "csk_conv2d_gn", _p(out) if keep_raw else None, _p(x),
                      _p(wf if xseg else wp), _p(bias), _p(bias2d), b2s,
                      _p(residual), B, H, W, Cin, Cout, kh, kw, stride, pt, pl, Ho, Wo, int(bool(up2x)), xs, ys, rs,
                      float(out_scale), int(dilation), tile, split, _p(ws), _p(yn), _p(gamma), _p(beta), int(groups),
                      float(eps), int(bool(silu)), int(bool(keep_raw)), *sargs, _s())
            SKGN_STATS[0] += 1
            if SKGN_SITES is not None:
                SKGN_SITES.append((B, Ho, Wo, Cin, Cout, split, bool(keep_raw)))
            return (yn, out) if keep_raw else yn
    seg = _gn_seg(tile, split, Ho * Wo, M, code, Cout) if gn_stats and ys == Cout else 0
    part = _gn_part(M, Cout, seg, x.device) if seg else None
    run(tile, split, part)
    if part is not None:
        out._csk_gn = (part, seg)
    return _norm_after(out, norm, norm_optional)


def _norm_after(out, norm, optional=False):
    """conv2d's ``norm`` argument where the conv kernel did not apply it"""
    if norm is None:
        return out
    gamma, beta, groups, eps, silu, keep_raw = norm
    if optional and keep_raw:
        SKGN_STATS[2] += 1
        return None, out
    SKGN_STATS[1] += 1
    yn = group_norm(out, gamma, beta, groups, eps, silu)
    return (yn, out) if keep_raw else yn


def _conv2d_u8(x, wp, bias, stride, padding, residual, up2x, bias2d, act, out_scale, out, dilation, residual2,
               res_scale, Ho, Wo):
    """conv2d with a uint8 image output (``out``: None or a contiguous uint8 [B, Ho, Wo, Cout])."""
    from . import norm_padding

    B, H, W, Cin = x.shape
    Cout = wp.shape[0]
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.uint8, device=x.device)
    if out.dtype != torch.uint8 or out.shape != (B, Ho, Wo, Cout) or not out.is_contiguous():
        raise ValueError("conv2d out_u8: out must be a contiguous uint8 [B, Ho, Wo, Cout]")
    xs = _pix_stride(x)
    if (CONV_TILE and Cout < 16 and residual is None and residual2 is None and bias2d is None and stride == 1
            and wp.shape[1:3] == (3, 3) and norm_padding(padding) == (1, 1, 1, 1) and dilation == 1
            and code_ok(act) and B * Ho * Wo >= CONV_TILE_NARROW_MIN_PX and xs is not None
            and x.data_ptr() % 16 == 0 and wp.is_contiguous() and wp.data_ptr() % 16 == 0
            and _lib.call_int("csk_conv_tile_ok2", B, Ho, Wo, Cin, Cout, xs, Cout, int(bool(up2x))) > 0):
        _lib.call("csk_conv_tile2", _p(out), _p(x), _p(wp), _p(bias), None, None, B, Ho, Wo, Cin, Cout, xs, Cout,
                  0, 0, ACT[act], float(out_scale), 1.0, int(bool(up2x)), 1, _s())
        CONV_TILE_STATS[0] += 1
        return out
    y = conv2d(x, wp, bias, stride, padding, residual, up2x, bias2d, act, out_scale, None, dilation,
               residual2=residual2, res_scale=res_scale)
    out.copy_((y.float().clamp(0, 1) * 255).round().to(torch.uint8))
    return out


def code_ok(act):
    """activations the halo-tile kernel's epilogue applies"""
    return ACT[act] in (0, 2, 5, 6, 8, 9)


# Depthwise NHWC conv and its stride-2 transpose (csrc/kernels/dwconv.hip)
sig("csk_dwconv_tile", c_int)
sig("csk_dwconv", c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p)
sig("csk_dwconv_t", c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p)
# dwconv.hip DW_TH / DW_TW / 8 * DW_CV: the output tile and channel block of one workgroup
DWCONV_TH, DWCONV_TW, DWCONV_CB = 8, 16, 64
DWCONV_VARIANTS = ("direct", "halo")
DWCONV_STATS = [0]  # kernel launches (tests assert the kernel ran)


def _dw_variant(kh, kw, stride):
    """Forward variant, as measured (tools/dwconvbench.py, profiles/dwconv_r8.txt):
    the LDS halo leads the 7x7 stride-1 conv by 0.5-1 us at every ConvNeXt
    shape; the 4x4 stride-2 binomial is faster straight from L2 (6.4 vs 9.8 us
    at 128^2 x 384), so stride 2 runs direct."""
    return "halo" if stride == 1 and kh * kw > 1 else "direct"


def _dw_operand(name, what, t, C):
    """Pixel stride of an NHWC operand (bf16, channel slices allowed)."""
    if t.dtype != torch.bfloat16:
        raise ValueError(f"{name}: {what} must be bfloat16 on the HIP path, got {t.dtype}")
    ps = _pix_stride(t)
    if ps is None or ps % 8 or ps < C or t.data_ptr() % 16:
        raise ValueError(f"{name}: {what} must be an NHWC tensor or channel slice (last dim contiguous, pixel "
                         f"stride and channel offset multiples of 8), got strides {t.stride()}")
    return ps


def _dw_common(name, x, wp, bias, out, ho, wo):
    B, H, W, C = x.shape
    xs = _dw_operand(name, "x", x, C)
    if not wp.is_cuda or wp.device != x.device or not wp.is_contiguous():
        raise ValueError(f"{name}: wp must be a contiguous tensor on {x.device}")
    if B > 65535:
        raise ValueError(f"{name}: batch {B} > 65535")
    bias_f32 = 0
    if bias is not None:
        if bias.dtype not in (torch.bfloat16, torch.float32) or not bias.is_contiguous() or bias.device != x.device:
            raise ValueError(f"{name}: bias must be contiguous bf16 or fp32 on {x.device}")
        if bias.data_ptr() % 16:
            raise ValueError(f"{name}: bias must be 16-byte aligned")
        bias_f32 = int(bias.dtype == torch.float32)
    if out is None:
        out = torch.empty((B, ho, wo, C), dtype=torch.bfloat16, device=x.device)
    os_ = _dw_operand(name, "out", out, C)
    return xs, os_, bias_f32, out


def depthwise_conv2d(x, wp, bias, stride, pad, pad_mode, residual, out, out_hw, variant=None):
    """``ops.depthwise_conv2d`` on the HIP kernel (arguments already validated
    there: ``pad`` is the 4-tuple, ``out_hw`` the output size).  ``variant``:
    "halo" / "direct", default ``_dw_variant``."""
    name = "depthwise_conv2d"
    B, H, W, C = x.shape
    ho, wo = out_hw
    kh, kw = wp.shape[0], wp.shape[1]
    xs, os_, bias_f32, out = _dw_common(name, x, wp, bias, out, ho, wo)
    rs = 0
    if residual is not None:
        rs = _dw_operand(name, "residual", residual, C)
    variant = variant or _dw_variant(kh, kw, stride)
    if variant not in DWCONV_VARIANTS:
        raise ValueError(f"{name}: variant {variant!r} not in {DWCONV_VARIANTS}")
    _lib.call("csk_dwconv", _p(x), _p(wp), _p(bias), bias_f32, _p(residual), _p(out), B, H, W, C, xs, rs, os_, ho, wo,
              kh, kw, int(stride), pad[0], pad[1], int(pad_mode == "reflect"), DWCONV_VARIANTS.index(variant), _s())
    DWCONV_STATS[0] += 1
    return out


def depthwise_conv_transpose2d(x, wp, bias, pad, pad_mode, crop, out, out_hw):
    """``ops.depthwise_conv_transpose2d`` on the HIP gather kernel."""
    name = "depthwise_conv_transpose2d"
    B, H, W, C = x.shape
    ho, wo = out_hw
    xs, os_, bias_f32, out = _dw_common(name, x, wp, bias, out, ho, wo)
    pt, pl, pb, pr = pad
    _lib.call("csk_dwconv_t", _p(x), _p(wp), _p(bias), bias_f32, _p(out), B, H, W, C, xs, os_, ho, wo, wp.shape[0],
              wp.shape[1], pt, pl, H + pt + pb, W + pl + pr, int(crop), int(pad_mode == "reflect"), _s())
    DWCONV_STATS[0] += 1
    return out


sig("csk_axpby_nhwc", c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_float, c_float, c_int,
    c_void_p)


def axpby_nhwc(x, z, a, b, out, act=None):
    """out = act(a*x + b*z) on NHWC channel-slice views (in place allowed; z may be None)."""
    xs, ys = _pix_stride(x), _pix_stride(out)
    zs = _pix_stride(z) if z is not None else 0
    if None in (xs, zs, ys) or (z is not None and x.shape != z.shape) or x.shape != out.shape:
        raise ValueError("axpby_nhwc: operands must be same-shape NHWC views")
    C = x.shape[-1]
    P = x.numel() // C
    if C % 8 or xs % 8 or ys % 8 or zs % 8:
        raise ValueError("axpby_nhwc: channels / pixel strides must be multiples of 8")
    _lib.call("csk_axpby_nhwc", _p(out), ys, _p(x), xs, _p(z), zs, P, C, float(a), float(b), ACT[act], _s())
    return out


def axpby(x, y, a, b, out=None):
    """out = a*x + b*y (bf16, contiguous)."""
    x, y = x.contiguous(), y.contiguous()
    out = torch.empty_like(x) if out is None else out
    _lib.call("csk_axpby", _p(out), _p(x), _p(y), x.numel(), float(a), float(b), _s())
    return out


def group_norm(x, gamma, beta, groups, eps, silu):
    _bf16(x, "group_norm.x")
    x = x.contiguous()
    B, C = x.shape[0], x.shape[-1]
    P = x.numel() // (B * C)
    # a chunk gives every thread >= 4 independent row loads (the kernels' unroll;
    # R = 256 threads / (C/8 vector columns) rows per pass), with <= ~1024
    # workgroups over the whole tensor (each apply workgroup re-merges the
    # statistics partials in its prologue: fewer, longer workgroups amortise it)
    rows = max(1, 256 // max(1, -(-(C // 8) // (2 if C > 2048 else 1))))
    chunk = max(4 * rows, -(-P * B // GN_TARGET_WG))
    nchunk = -(-P // chunk)
    chunk = -(-P // nchunk)
    bstride = 0
    if gamma.dim() == 2:
        if gamma.shape != (B, C) or beta.shape != (B, C):
            raise ValueError("group_norm: per-sample affine must be [B, C]")
        # rows of a wider matrix (e.g. slices of one batched projection) are
        # read in place when both share the row stride
        if gamma.stride(1) != 1 or beta.stride(1) != 1 or gamma.stride(0) != beta.stride(0):
            gamma, beta = gamma.contiguous(), beta.contiguous()
        bstride = gamma.stride(0)
    act = 2 if silu == "gelu" else int(bool(silu))
    y = torch.empty_like(x)
    fused = getattr(x, "_csk_gn", None)
    if fused is not None:
        fpart, seg = fused
        if P % seg == 0 and fpart.numel() == (B * P // seg) * C * 2:
            stat = torch.empty(B * groups * 2, dtype=torch.float32, device=x.device)
            _lib.call("csk_group_norm_part", _p(y), _p(x), None, 0, _p(fpart), seg, _p(stat), _p(gamma), _p(beta),
                      B, P, C, groups, chunk, nchunk, float(eps), act, bstride, _s())
            return y
    part = torch.empty(B * nchunk * groups * 3 + B * groups * 2, dtype=torch.float32, device=x.device)
    _lib.call("csk_group_norm", _p(y), _p(x), None, 0, _p(part), _p(gamma), _p(beta), B, P, C, groups, chunk, nchunk,
              float(eps), act, bstride, _s())
    return y


def group_norm_cat(a, b, gamma, beta, groups, eps, silu):
    """GroupNorm(+SiLU) of the channel concat [a | b] without materialising it
    (UNet skip connections): the apply kernel reads both tensors in place.
    Needs the fused epilogue statistics of both (same segment height);
    returns None otherwise (the caller concatenates)."""
    sa, sb = getattr(a, "_csk_gn", None), getattr(b, "_csk_gn", None)
    GN_CAT_STATS[1] += 1
    if a.shape[:-1] != b.shape[:-1] or not (a.is_contiguous() and b.is_contiguous()):
        return None
    B, Ca, Cb = a.shape[0], a.shape[-1], b.shape[-1]
    C = Ca + Cb
    P = a.numel() // (B * Ca)
    if Ca % 8 or Cb % 8 or gamma.dim() != 1 or C % groups or C > 4096:
        return None
    rows = max(1, 256 // max(1, -(-(C // 8) // (2 if C > 2048 else 1))))
    chunk = max(4 * rows, -(-P * B // GN_TARGET_WG))
    nchunk = -(-P // chunk)
    chunk = -(-P // nchunk)
    y = torch.empty(a.shape[:-1] + (C,), dtype=torch.bfloat16, device=a.device)
    fused = sa is not None and sb is not None and sa[1] == sb[1] and P % sa[1] == 0
    if fused:
        seg = sa[1]
        nseg = sa[0].numel() // (2 * Ca)
        fused = nseg * 2 * Cb == sb[0].numel()
    if fused:  # both producers emitted epilogue statistics: merged from both buffers in place
        stat = torch.empty(B * groups * 2, dtype=torch.float32, device=a.device)
        _lib.call("csk_group_norm_part2", _p(y), _p(a), _p(b), Ca, _p(sa[0]), _p(sb[0]), seg, _p(stat), _p(gamma),
                  _p(beta), B, P, C, groups, chunk, nchunk, float(eps), int(bool(silu)), 0, _s())
    else:  # statistics pass over both tensors in place (e.g. a split-K producer)
        part = torch.empty(B * nchunk * groups * 3 + B * groups * 2, dtype=torch.float32, device=a.device)
        _lib.call("csk_group_norm", _p(y), _p(a), _p(b), Ca, _p(part), _p(gamma), _p(beta), B, P, C, groups, chunk,
                  nchunk, float(eps), int(bool(silu)), 0, _s())
    GN_CAT_STATS[0] += 1
    return y


GN_CAT_STATS = [0, 0]  # (concats normalised in place, attempts)


def layer_norm(x, gamma, beta, eps):
    _bf16(x, "layer_norm.x")
    x = x.contiguous()
    C = x.shape[-1]
    y = torch.empty_like(x)
    _lib.call("csk_layer_norm", _p(y), _p(x), _p(gamma), _p(beta), x.numel() // C, C, float(eps), _s())
    return y


def attention(q, k, v, scale, causal=False, kv_len=None):
    """``kv_len``: optional int32 device tensor [1] = number of valid keys
    (<= k.shape[1]), read by the kernel (graph-capturable KV-cache decode)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _bf16(t, "attention." + n)
        if t.stride(-1) != 1:
            raise ValueError("attention: last dim must be contiguous")
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    if D > 512 or (D > 256 and (causal or kv_len is not None or D % 16)):
        raise ValueError(f"attention: head dim {D} unsupported (<= 256, or <= 512 non-causal, multiple of 16)")
    o = torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=q.device)
    st = (c_int64 * 12)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o.stride()[:3])
    if kv_len is not None and (kv_len.dtype != torch.int32 or not kv_len.is_cuda):
        raise TypeError("attention: kv_len must be an int32 device tensor")
    plain = not causal and kv_len is None and ATTN_VARIANT == 0
    if plain and attn_fa_ok(B, H, Sq, Skv, D):  # persistent stream-K kernel (no split path needed)
        _lib.call("csk_attention_fa", _p(o), _p(q), _p(k), _p(v), st, B, H, Sq, Skv, D, float(scale), ATTN_FA_WORKERS,
                  _s())
        return o
    split = attn_kv_split(B, H, Sq, Skv, D) if plain else 1
    if split > 1:
        return attention_split(q, k, v, scale, split, o)
    _lib.call("csk_attention", _p(o), _p(q), _p(k), _p(v), st, B, H, Sq, Skv, D, float(scale), int(bool(causal)),
              ATTN_VARIANT, _p(kv_len), _s())
    return o


sig("csk_attention_bias", c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_int, c_int, c_int, c_int,
    c_int, c_float, c_int, c_void_p, ctypes.POINTER(c_int64), c_void_p, c_void_p)
sig("csk_set_attn_bias_waves", c_int)


def set_attn_bias_waves(n: int):
    """Waves per workgroup of the bias / key-length attention: 0 auto, 1 / 2 / 4
    (16 query rows per wave; A/B knob of tools/attnbiasbench.py)."""
    _lib.call("csk_set_attn_bias_waves", int(n))


def attention_bias(q, k, v, scale, causal=False, bias=None, kv_lens=None):
    """softmax(q k^T * scale + bias) v over each sample's first ``kv_lens[b]``
    keys (csrc/kernels/attn_bias.hip).  ``bias``: fp32 device tensor
    broadcastable to [B, H, Sq, Skv] (expanded here: broadcast dims become
    stride 0); ``kv_lens``: int32 device tensor [B], read by the kernel.  No
    host read, no allocation but the output: graph-capturable."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _bf16(t, "attention_bias." + n)
        if t.dim() != 4:
            raise ValueError(f"attention_bias.{n}: expected [B, S, H, D], got {tuple(t.shape)}")
        if not t.is_cuda:
            raise TypeError(f"attention_bias.{n}: must be a device tensor")
        if t.stride(-1) != 1:
            raise ValueError("attention_bias: last dim must be contiguous")
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    if k.shape != (B, Skv, H, D) or v.shape != (B, Skv, H, D):
        raise ValueError(f"attention_bias: k / v {tuple(k.shape)} / {tuple(v.shape)} do not match q {tuple(q.shape)}")
    if bias is not None:
        if bias.dtype != torch.float32 or not bias.is_cuda:
            raise TypeError("attention_bias: bias must be a float32 device tensor")
        if bias.dim() == 0:
            bias = bias.reshape(1)
        full = (B, H, Sq, Skv)
        if bias.dim() > 4 or any(n not in (1, m) for n, m in zip(bias.shape[::-1], full[::-1])):
            raise ValueError(f"attention_bias: bias {tuple(bias.shape)} does not broadcast to {full}")
        if Skv > 1 and (bias.shape[-1] != Skv or bias.stride(-1) != 1):
            bias = bias.expand(*bias.shape[:-1], Skv).contiguous()  # the kernel reads 4 consecutive keys
        bias = bias.expand(B, H, Sq, Skv)
    if kv_lens is not None:
        if kv_lens.dtype != torch.int32 or not kv_lens.is_cuda:
            raise TypeError("attention_bias: kv_lens must be an int32 device tensor")
        if tuple(kv_lens.shape) != (B,) or kv_lens.stride(0) != 1:
            raise ValueError(f"attention_bias: kv_lens must be a contiguous [B = {B}] tensor, got {tuple(kv_lens.shape)}")
    if D > 128 or D % 8 or D < 8:  # shapes the kernel does not take: the reference formula on the device
        from . import _ref_attention_bias

        return _ref_attention_bias(q, k, v, scale, causal, bias, kv_lens)
    o = torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=q.device)
    if o.numel() == 0:
        return o
    if Skv == 0:
        return o.zero_()
    st = (c_int64 * 12)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o.stride()[:3])
    bst = (c_int64 * 3)(*bias.stride()[:3]) if bias is not None else None
    _lib.call("csk_attention_bias", _p(o), _p(q), _p(k), _p(v), st, B, H, Sq, Skv, D, float(scale),
              int(bool(causal)), _p(bias), bst, _p(kv_lens), _s())
    return o


def attention_split(q, k, v, scale, split, o=None):
    """d = 64 non-causal attention with the keys split over ``split`` workgroups
    per query block (fp32 partials in a torch workspace, then a combine pass)."""
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    if D != 64 or not 2 <= split <= 16:
        raise ValueError("attention_split: head dim 64, 2..16 splits")
    if o is None:
        o = torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=q.device)
    st = (c_int64 * 12)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o.stride()[:3])
    rows = B * H * Sq
    part_o = torch.empty((split, rows, 64), dtype=torch.float32, device=q.device)
    part_ml = torch.empty((split, rows, 2), dtype=torch.float32, device=q.device)
    _lib.call("csk_attention_split", _p(o), _p(q), _p(k), _p(v), st, B, H, Sq, Skv, D, float(scale), split,
              _p(part_o), _p(part_ml), _s())
    return o


ATTN_FA = os.environ.get("CSK_ATTN_FA", "1") == "1"  # mirrors csk_set_attn_fa (set_attn_fa)
ATTN_FA_WORKERS = 0  # 0: one persistent workgroup per CU; tests pass fewer to force more stream-K cuts


def attn_fa_ok(B, H, Sq, Skv, D) -> bool:
    """Shapes the persistent stream-K d = 64 attention (csrc/kernels/attn_fa.hip) takes."""
    return ATTN_FA and _lib.call_int("csk_attn_fa_ok", B, H, Sq, Skv, D, 0, 0) == 1


def set_attn_fa(on: bool):
    global ATTN_FA
    ATTN_FA = bool(on)
    _lib.call("csk_set_attn_fa", int(ATTN_FA))


def attn_fa_errors() -> int:
    """Merge-protocol spins that gave up since the library loaded (must stay 0)."""
    out = ctypes.c_uint(0)
    fn = _lib.load().csk_attn_fa_errors
    fn.restype = ctypes.c_int
    err = fn(ctypes.byref(out))
    if err:
        raise RuntimeError(f"csk_attn_fa_errors: hipError {err}")
    return int(out.value)


sig("csk_attn_fa_reset")


def attn_fa_health() -> bool:
    """Per-job check of the stream-K attention's merge protocol (called by
    runtime/device.py after every GPU job).  A spin that gave up means a late
    contributor may publish into a slot after its owner released it, so the
    partials of every later launch are suspect: the kernel is switched off for
    this process, its flags are zeroed, and False is returned (the caller fails
    the job and drops the captured graphs, which still launch the kernel)."""
    if attn_fa_errors() == 0:
        return True
    set_attn_fa(False)
    _lib.call("csk_attn_fa_reset")
    return False


ATTN32 = True  # mirrors the library's csk_set_attn32 (set_attn32): the split-KV path runs attn32_kernel only


def set_attn32(on: bool):
    """Turn the 32x32x16 self-attention kernel on / off (A/B and fallback
    switch) in the library AND here: with it off, the key-split path (which
    always runs attn32_kernel) is skipped too."""
    global ATTN32
    ATTN32 = bool(on)
    _lib.call("csk_set_attn32", int(ATTN32))


ATTN_SPLIT_WG = int(os.environ.get("CSK_ATTN_SPLIT_WG", "1024"))  # split the keys below this many workgroups (0: off); 1024 vs 512: -0.045 ms/step at CFG batch 2 (profiles/unet_step_ab_attn_split_wg_b2_r5p.txt)


def attn_kv_split(B, H, Sq, Skv, D) -> int:
    """Key splits for the d = 64 self-attention when its 128-query workgroups
    cannot fill the chip (batch-1 jobs): up to 4."""
    if D != 64 or Skv <= 128 or ATTN_SPLIT_WG <= 0 or not ATTN32:
        return 1
    wg = B * H * -(-Sq // 128)
    split = 1
    # each split keeps >= 16 key blocks: at S = 1024 (16 blocks) the combine and
    # the shorter pipelines cost more than the extra workgroups gain (30.6 vs
    # 22.5 us, profiles/attn_split_r4t.txt); S = 4096 at batch 1-2: 58 vs 75 us
    while wg * split < ATTN_SPLIT_WG and split < 4 and -(-Skv // 64) >= 32 * split:
        split *= 2
    return split


def silu(x):
    """Any length: the kernel does 8-element vectors plus a scalar tail."""
    _bf16(x, "silu")
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.call("csk_silu", _p(y), _p(x), x.numel(), _s())
    return y


def row_bcast(dst, tab, cur):
    """dst[r] = tab[cur[0]] for every row r (bf16 [rows, W] <- [n, W], int32 device index)."""
    _bf16(dst, "row_bcast.dst")
    _bf16(tab, "row_bcast.tab")
    if dst.dim() != 2 or tab.dim() != 2 or dst.shape[1] != tab.shape[1] or not dst.is_contiguous() \
            or not tab.is_contiguous() or cur.dtype != torch.int32:
        raise ValueError("row_bcast: contiguous bf16 [rows, W] / [n, W], int32 cur")
    _lib.call("csk_row_bcast", _p(dst), _p(tab), _p(cur), dst.shape[0], dst.shape[1], tab.shape[0], _s())


def dup2(x):
    """[x; x] along dim 0 (CFG-shared prefix -> both guidance halves) in one pass."""
    x = x.contiguous()
    y = torch.empty((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    if x.dtype != torch.bfloat16 or x.numel() % 8 or x.data_ptr() % 16:
        y[: x.shape[0]].copy_(x)
        y[x.shape[0]:].copy_(x)
        return y
    _lib.call("csk_dup2", _p(y), _p(x), x.numel(), _s())
    return y


def add(x, y):
    _bf16(x, "add")
    if x.shape != y.shape:
        raise ValueError(f"hip add: shapes {tuple(x.shape)} and {tuple(y.shape)} differ (no broadcasting)")
    x, y = x.contiguous(), y.contiguous().to(x.dtype)
    out = torch.empty_like(x)
    _lib.call("csk_add", _p(out), _p(x), _p(y), x.numel(), _s())
    return out


def sched_step(e, x, prev_x0, c, guidance, noise):
    _bf16(e, "sched_step.e")
    x = x.contiguous()
    n = x.numel()
    cfg = guidance is not None
    if e.numel() != n * (2 if cfg else 1):
        raise ValueError("sched_step: model output / latent size mismatch")
    xn = torch.empty_like(x)
    x0 = torch.empty_like(x)
    _lib.call("csk_sched_step", _p(xn), _p(x0), _p(e.contiguous()), _p(x),
              _p(prev_x0) if (prev_x0 is not None and c.C != 0.0) else None,
              _p(noise) if (noise is not None and c.D != 0.0) else None, n,
              float(c.p), float(c.q), float(c.A), float(c.B), float(c.C), float(c.D),
              float(guidance or 0.0), int(cfg), _s())
    return xn, x0


def loop_prologue(counter, cur, t_tab, t_out):
    """Head of a device-resident sampler step: cur = counter++, t_out = t_tab[cur]
    (int32 [1] counter / cur, fp32 table, fp32 [1] output; 1-thread kernel)."""
    if counter.dtype != torch.int32 or cur.dtype != torch.int32 or t_tab.dtype != torch.float32 \
            or t_out.dtype != torch.float32 or t_tab.numel() < 1:
        raise TypeError("loop_prologue: int32 counter/cur, fp32 t_tab/t_out")
    _lib.call("csk_loop_prologue", _p(counter), _p(cur), _p(t_tab), _p(t_out), t_tab.numel(), _s())


def sched_loop(e, x, x0prev, noise_tab, cur, coef, x_in, mode, reps=None):
    """Tail of a device-resident sampler step (elementwise.hip sched_loop_kernel):
    CFG combine (mode 0 none, 1 [u, c], 2 pix2pix [c, i, u]) + the linear update
    with the coefficients of step ``cur`` from the device table ``coef``
    [n, LOOP_COEF_STRIDE] (guidance scales in the row),
    x / x0prev updated in place, the next UNet input written into ``x_in``
    ([reps * B, H, W, Cin] bf16, channels 0..3 of every replica; reps defaults
    to the CFG replica count, 1 for a CFG-parallel half)."""
    _bf16(e, "sched_loop.e")
    _bf16(x_in, "sched_loop.x_in")
    nrep = mode + 1
    reps = nrep if reps is None else int(reps)
    B, H, W, C = x.shape
    if C != 4 or x.dtype != torch.float32 or not x.is_contiguous() or not x0prev.is_contiguous() \
            or x0prev.shape != x.shape or x0prev.dtype != torch.float32:
        raise ValueError("sched_loop: x / x0prev must be contiguous fp32 [B, H, W, 4]")
    if e.numel() != nrep * x.numel() or not e.is_contiguous():
        raise ValueError(f"sched_loop: model output {tuple(e.shape)} vs {nrep} x {tuple(x.shape)}")
    if x_in.dim() != 4 or x_in.shape[0] != reps * B or x_in.shape[1:3] != (H, W) or x_in.shape[3] < 4 \
            or not x_in.is_contiguous():
        raise ValueError(f"sched_loop: x_in {tuple(x_in.shape)} for {reps} x {tuple(x.shape)}")
    if coef.dtype != torch.float32 or coef.dim() != 2 or coef.shape[1] != LOOP_COEF_STRIDE \
            or cur.dtype != torch.int32:
        raise ValueError("sched_loop: coef must be fp32 [n, LOOP_COEF_STRIDE], cur int32")
    if noise_tab is not None and (noise_tab.dtype != torch.float32 or
                                  noise_tab.numel() != coef.shape[0] * x.numel()):
        raise ValueError("sched_loop: noise table must be fp32 [n, B, H, W, 4]")
    _lib.call("csk_sched_loop", _p(e), _p(x), _p(x0prev), _p(noise_tab), _p(cur), _p(coef), _p(x_in),
              x_in.shape[3], reps, B * H * W, mode, _s())


def vae_postprocess(img):
    _bf16(img, "vae_post")
    img = img.contiguous()
    y = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
    _lib.call("csk_vae_post", _p(y), _p(img), img.numel(), _s())
    return y


def canny(img, low, high):
    """uint8 [H, W] or [H, W, C] device image -> uint8 0/255 edge map [H, W]
    (csrc/kernels/canny.hip; multi-channel: cv2's per-pixel max-gradient channel)."""
    if img.dtype != torch.uint8 or img.dim() not in (2, 3):
        raise TypeError("canny: uint8 [H, W] or [H, W, C] expected")
    img = img.contiguous()
    H, W = img.shape[:2]
    C = 1 if img.dim() == 2 else img.shape[2]
    out = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    a4, a1 = -(-(H * W * 4) // 256) * 256, -(-(H * W) // 256) * 256
    ws = torch.empty(256 + a4 + 2 * a1, dtype=torch.uint8, device=img.device)  # torch: 256 B-aligned
    _lib.call("csk_canny", _p(out), _p(img), H, W, C, float(low), float(high), _p(ws), _s())
    return out


XATTN_FUSED = os.environ.get("CSK_XATTN", "1") == "1"  # fused cross-attention sub-block (csrc/kernels/xattn.hip)
XATTN_CHANNELS = (320,)
# workgroup shape of the fused kernel: 4 waves x 32 rows or 8 waves x 16 rows (csk_set_xattn_waves)
XATTN_WAVES = int(os.environ.get("CSK_XATTN_WAVES", "8"))  # 8: 40 vs 50 us, profiles/xattnbench_waves_r6h.txt
_xattn_waves_applied = [None]


# below this many 128-row workgroups the fused kernel (one workgroup per CU)
# leaves CUs idle and the unfused Q GEMM + short-KV attention + out GEMM chain
# wins: CFG batch 2 (64 workgroups) 5.632 vs 5.679 ms per step unfused / fused,
# CFG batch 8 (256) 11.765 vs 11.799 fused / unfused (profiles/unet_step_ab_xattn_gate_r7j.txt)
XATTN_MIN_WG = int(os.environ.get("CSK_XATTN_MIN_WG", "256"))


def xattn_ok(x, kv, rows_per_b) -> bool:
    """Shapes the fused cross-attention sub-block kernel takes: C = 320 (5 heads
    of 64), <= 80 context tokens, whole 128-row tiles of one sample, and a grid
    of at least XATTN_MIN_WG workgroups."""
    C = x.shape[-1]
    return _xattn_rows_ok(x.numel() // max(C, 1), C, kv, rows_per_b)


def _xattn_rows_ok(M, C, kv, rows_per_b) -> bool:
    if M // 128 < XATTN_MIN_WG:
        return False
    return (XATTN_FUSED and C in XATTN_CHANNELS and kv is not None and kv.dim() == 5 and kv.shape[2] == 2
            and kv.shape[3] * kv.shape[4] == C and kv.shape[4] == 64 and 1 <= kv.shape[1] <= 80
            and rows_per_b % 128 == 0 and M % rows_per_b == 0
            and kv.shape[0] >= M // rows_per_b)


# The self-attention out-projection as the prologue of the fused block
# (xattn.hip, PRE variant): x = bf16(h0 + O Wo1^T + bo1) is formed in registers
# and never stored.  CSK_XATTN_PRE=0: the out-projection stays its own GEMM.
# CSK_XATTN_DUP=0: the CFG-shared first block (both halves from the half-batch
# self-attention, source row m % src_rows) keeps the unfused chain.
# (tools/abstep.py arms xpre0 / xpre1, xdup0 / xdup1)
sig("csk_xattn_block_pre_ok", c_int, c_int, c_int, c_int, c_int, c_int)
sig("csk_xattn_block_pre", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
    c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p)
XATTN_PRE = os.environ.get("CSK_XATTN_PRE", "1") == "1"
XATTN_DUP = os.environ.get("CSK_XATTN_DUP", "1") == "1"
XATTN_PRE_STATS = [0]  # calls with the prologue, same batch (tests assert the fused path ran)
XATTN_DUP_STATS = [0]  # calls with the prologue that also double the batch


def xattn_pre_ok(o, kv, rows_per_b, dup=False) -> bool:
    """``xattn_ok`` for the block whose input the prologue forms from the
    attention output ``o`` [b, S, C] (``dup``: for twice the batch)."""
    if not XATTN_PRE or (dup and not XATTN_DUP) or o.dim() != 3 or o.dtype != torch.bfloat16:
        return False
    b, s, c = o.shape
    return _xattn_rows_ok((2 * b if dup else b) * s, c, kv, rows_per_b)


def _xattn_block_pre(pre, batch, wq, colsum, bq, kv, wo, bo, eps, scale, rows_per_b, row_stats):
    o, h0, wo1, bo1 = pre
    for t, n in ((o, "o"), (h0, "h0"), (wo1, "wo1"), (wq, "wq"), (bq, "bq"), (kv, "kv"), (wo, "wo")):
        _bf16(t, "xattn_block.pre." + n)
    for t, n in ((bo1, "bo1"), (bo, "bo")):
        if t is not None:
            _bf16(t, "xattn_block.pre." + n)
    b, s, C = o.shape
    batch = b if batch is None else int(batch)
    if h0.shape != o.shape or tuple(wo1.shape) != (C, C) or batch % b:
        raise ValueError(f"xattn_block: prologue operands {tuple(o.shape)} / {tuple(h0.shape)} / {tuple(wo1.shape)} "
                         f"do not match batch {batch}")
    src_rows, M = b * s, batch * s
    kv = kv.contiguous()
    if colsum.dtype != torch.float32 or colsum.numel() != C:
        raise ValueError("xattn_block: colsum must be fp32 [C]")
    if _lib.call_int("csk_xattn_block_pre_ok", M, C, int(rows_per_b), int(kv.shape[0]), int(kv.shape[1]),
                     src_rows) != 1:
        raise ValueError(f"xattn_block: unsupported prologue shape M={M} C={C} rows/sample={rows_per_b} "
                         f"kv={tuple(kv.shape)} source rows={src_rows}")
    y = torch.empty((batch, s, C), dtype=torch.bfloat16, device=o.device)
    rp = torch.empty(M * 2, dtype=torch.float32, device=o.device) if row_stats else None
    (XATTN_DUP_STATS if batch != b else XATTN_PRE_STATS)[0] += 1
    _lib.call("csk_xattn_block_pre", _p(y), _p(o.contiguous()), _p(h0.contiguous()), _p(wo1.contiguous()),
              _p(None if bo1 is None else bo1.contiguous()), _p(wq.contiguous()), _p(colsum.contiguous()),
              _p(bq.contiguous()), _p(kv), _p(wo.contiguous()), _p(None if bo is None else bo.contiguous()), _p(rp),
              M, C, int(rows_per_b), int(kv.shape[0]), int(kv.shape[1]), src_rows, float(eps), float(scale), _s())
    if rp is not None:
        y._csk_rows = (rp, 1, C)
    return y


def xattn_block(x, wq, colsum, bq, kv, wo, bo, eps, scale, rows_per_b, row_stats=True, pre=None, batch=None):
    """y = x + softmax((LN(x) Wq^T) scale K^T) V Wo^T + bo in ONE kernel
    (LayerNorm folded into ``wq`` / ``colsum`` / ``bq``: ops.fold_layer_norm).
    x: [B, S, C] bf16; kv: [Bc, Skv, 2, H, 64] (Attention.context_kv).  With
    ``row_stats`` the output carries ``_csk_rows`` = (part, 1, C) for the next
    fused LayerNorm.
    ``pre = (o, h0, wo1, bo1)`` (then ``x`` is None): x = h0 + o wo1^T + bo1 is
    formed in the kernel's prologue — ``wq`` must then be column-permuted by
    ``ops.permute_xattn_q`` — for ``batch`` samples (default: those of ``o``; a
    multiple repeats ``o`` / ``h0``, the K/V differ)."""
    if pre is not None:
        return _xattn_block_pre(pre, batch, wq, colsum, bq, kv, wo, bo, eps, scale, rows_per_b, row_stats)
    for t, n in ((x, "x"), (wq, "wq"), (bq, "bq"), (kv, "kv"), (wo, "wo")):
        _bf16(t, "xattn_block." + n)
    if bo is not None:
        _bf16(bo, "xattn_block.bo")
    C = x.shape[-1]
    M = x.numel() // C
    x2 = x.reshape(M, C)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    kv = kv.contiguous()
    if colsum.dtype != torch.float32 or colsum.numel() != C:
        raise ValueError("xattn_block: colsum must be fp32 [C]")
    y = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    rp = torch.empty(M * 2, dtype=torch.float32, device=x.device) if row_stats else None
    if _xattn_waves_applied[0] != XATTN_WAVES:
        _lib.call("csk_set_xattn_waves", int(XATTN_WAVES))
        _xattn_waves_applied[0] = XATTN_WAVES
    _lib.call("csk_xattn_block", _p(y), _p(x2), _p(wq.contiguous()), _p(colsum.contiguous()), _p(bq.contiguous()),
              _p(kv), _p(wo.contiguous()), _p(None if bo is None else bo.contiguous()), _p(rp), M, C, int(rows_per_b),
              int(kv.shape[0]), int(kv.shape[1]), float(eps), float(scale), _s())
    out = y.view(x.shape)
    if rp is not None:
        out._csk_rows = (rp, 1, C)
    return out


# Fused feed-forward (csrc/kernels/ff.hip): LN3 + GEGLU + down-projection +
# residual in one kernel at C = 320; the [M, 4C] intermediate stays on chip.
sig("csk_ff_geglu_ok", c_int, c_int, c_int)
sig("csk_ff_geglu", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
    c_int, c_float, c_void_p)
sig("csk_set_ff_probe", c_int)
# below this many rows (CFG batch 2 at 64x64: 8192) the 128-row workgroups
# leave most CUs idle and the two tuned GEMMs win (tools/ffbench.py)
FF_MIN_ROWS = int(os.environ.get("CSK_FF_MIN_ROWS", "16384"))
FF_FUSED = os.environ.get("CSK_FF_FUSED", "1") == "1"


def ff_fused_ok(x, inner: int) -> bool:
    C = x.shape[-1]
    M = x.numel() // C
    return (FF_FUSED and x.dtype == torch.bfloat16 and M >= FF_MIN_ROWS
            and _lib.call_int("csk_ff_geglu_ok", M, C, inner) == 1)


def ff_geglu(x, gamma, beta, w1p, b1p, w2p, b2, eps):
    """y = x + W2 GEGLU(W1 LayerNorm(x) + b1) + b2 in ONE kernel (C = 320).
    Weights packed by ``ops.pack_ff_fused`` (the kernel's LDS images, swizzle
    included): w1p [I/16, C/64, 32, 64] bf16, b1p [I/16, 32] fp32,
    w2p [I/32, C/32, 32, 32] bf16."""
    for t, n in ((x, "x"), (gamma, "gamma"), (w1p, "w1p"), (w2p, "w2p")):
        _bf16(t, "ff_geglu." + n)
    C = x.shape[-1]
    M = x.numel() // C
    inner = 32 * w2p.shape[0]
    x2 = x.reshape(M, C)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    if beta is not None:
        _bf16(beta, "ff_geglu.beta")
    if b2 is not None:
        _bf16(b2, "ff_geglu.b2")
    if b1p is not None and b1p.dtype != torch.float32:
        raise ValueError("ff_geglu: b1p must be fp32")
    _lib.call("csk_ff_geglu", _p(y), _p(x2), _p(gamma.contiguous()), _p(None if beta is None else beta.contiguous()),
              _p(w1p.contiguous()), _p(None if b1p is None else b1p.contiguous()), _p(w2p.contiguous()),
              _p(None if b2 is None else b2.contiguous()), M, C, inner, float(eps), _s())
    return y.view(x.shape)


# The transformer's proj_out in the tail of the fused feed-forward
# (ff.hip, PROJ variant): z = x_in + Wp bf16(ff(x)) + bp and the GroupNorm
# partials of z in the same kernel; the FF output never reaches HBM.
# CSK_FF_PROJ=0: proj_out stays its own GEMM (tools/abstep.py arms ffp0 / ffp1).
sig("csk_ff_geglu_proj_ok", c_int, c_int, c_int, c_int, c_int)
sig("csk_ff_geglu_proj", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
    c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p)
FF_PROJ = os.environ.get("CSK_FF_PROJ", "1") == "1"
FF_PROJ_STATS = [0]  # calls (tests assert the fused path ran)


def ff_proj_seg(M, C, gn_rows) -> int:
    """GroupNorm-statistics segment height the stand-alone proj_out GEMM
    [M, C] x [C, C] writes for this shape (``gemm``'s tile plan, ``_gn_seg``):
    the fused kernel emits the same one, so every consumer — ``group_norm_cat``
    wants equal segments of both operands — keeps the path it has."""
    hit = tuning._lookup(tuning.table(), f"g:{M}:{C}:{C}:0")
    tile, split = (int(hit[0]), int(hit[1])) if hit is not None else tuning.heuristic(M, C, C)
    if split < 0 and tile not in tuning.GLDS:
        split = 1
    return _gn_seg(tile, split, gn_rows, M, 0, C)


def ff_proj_ok(x, inner: int, gn_rows: int) -> int:
    """Segment height (32 / 64 / 128) when the fused FF + proj_out kernel takes
    this block, else 0."""
    C = x.shape[-1]
    M = x.numel() // C
    if not (FF_PROJ and ff_fused_ok(x, inner)):
        return 0
    seg = ff_proj_seg(M, C, gn_rows)
    if seg not in (32, 64, 128) or _lib.call_int("csk_ff_geglu_proj_ok", M, C, inner, seg, gn_rows) != 1:
        return 0
    return seg


def ff_geglu_proj(x, gamma, beta, w1p, b1p, w2p, b2, wpp, bp, xin, eps, gn_rows=0, seg=0):
    """z = xin + Wp bf16(x + W2 GEGLU(W1 LayerNorm(x) + b1) + b2) + bp in ONE
    kernel (C = 320, M a multiple of 128): ``ff_geglu`` with the C x C
    projection ``wpp`` (``ops.pack_ff_proj``) in its tail.  ``seg`` (32, 64 or
    128, dividing ``gn_rows`` = rows per sample): also the GroupNorm partials
    of z per ``seg`` rows, attached as ``z._csk_gn`` like ``gemm(gn_rows=)``."""
    for t, n in ((x, "x"), (gamma, "gamma"), (w1p, "w1p"), (w2p, "w2p"), (wpp, "wpp"), (xin, "xin")):
        _bf16(t, "ff_geglu_proj." + n)
    for t, n in ((beta, "beta"), (b2, "b2"), (bp, "bp")):
        if t is not None:
            _bf16(t, "ff_geglu_proj." + n)
    if b1p is not None and b1p.dtype != torch.float32:
        raise ValueError("ff_geglu_proj: b1p must be fp32")
    C = x.shape[-1]
    M = x.numel() // C
    inner = 32 * w2p.shape[0]
    if xin.numel() != M * C or tuple(wpp.shape) != (C // 32, C // 32, 32, 32):
        raise ValueError(f"ff_geglu_proj: residual {tuple(xin.shape)} / packed proj {tuple(wpp.shape)} do not match "
                         f"{tuple(x.shape)}")
    if _lib.call_int("csk_ff_geglu_proj_ok", M, C, inner, int(seg), int(gn_rows)) != 1:
        raise ValueError(f"ff_geglu_proj: unsupported shape M={M} C={C} I={inner} seg={seg} rows/sample={gn_rows}")
    x2, r2 = x.reshape(M, C), xin.reshape(M, C)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if not r2.is_contiguous():
        r2 = r2.contiguous()
    z = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    part = _gn_part(M, C, seg, x.device) if seg else None
    FF_PROJ_STATS[0] += 1
    _lib.call("csk_ff_geglu_proj", _p(z), _p(x2), _p(gamma.contiguous()),
              _p(None if beta is None else beta.contiguous()), _p(w1p.contiguous()),
              _p(None if b1p is None else b1p.contiguous()), _p(w2p.contiguous()),
              _p(None if b2 is None else b2.contiguous()), _p(wpp.contiguous()),
              _p(None if bp is None else bp.contiguous()), _p(r2), _p(part), int(seg), int(gn_rows), M, C, inner,
              float(eps), _s())
    z = z.view(xin.shape)
    if part is not None:
        z._csk_gn = (part, seg)
    return z


sig("csk_set_xattn_probe", c_int)
sig("csk_set_xattn_waves", c_int)


# Fused transformer input (csrc/kernels/xin.hip): GroupNorm apply + proj_in +
# LN1 + QKV projection in one kernel at C = 320; the normalised input stays in
# registers, h is stored once (the out-projection's residual).
sig("csk_xin_qkv_ok", c_int, c_int, c_int, c_int)
sig("csk_xin_qkv", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
    c_void_p, c_int, c_int, c_float, c_void_p)
sig("csk_set_xin_probe", c_int)
sig("csk_set_conv_tile_no_rw", c_int)
sig("csk_gn_finalize", c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p)
XIN_FUSED = os.environ.get("CSK_XIN_FUSED", "1") == "1"
XIN_MIN_ROWS = int(os.environ.get("CSK_XIN_MIN_ROWS", "16384"))  # CFG-2 grids (8192 rows: 64 workgroups) keep the GEMMs (tools/xinbench.py)


def gn_stats(x, groups, eps):
    """(mean, rstd) [B, G, 2] fp32 of a [B, ..., C] bf16 tensor from its
    producer's fused epilogue statistics (``x._csk_gn``), or None without them."""
    fused = getattr(x, "_csk_gn", None)
    if fused is None:
        return None
    B, C = x.shape[0], x.shape[-1]
    P = x.numel() // (B * C)
    part, seg = fused
    if P % seg or part.numel() != (B * P // seg) * C * 2 or C % groups:
        return None
    stat = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
    _lib.call("csk_gn_finalize", _p(stat), _p(part), None, 0, seg, B, P, C, groups, float(eps), _s())
    return stat


def xin_ok(x, groups) -> bool:
    """x: [B, P, C] (or NHWC) block input with fused GN statistics attached."""
    if not XIN_FUSED or x.dtype != torch.bfloat16 or getattr(x, "_csk_gn", None) is None:
        return False
    B, C = x.shape[0], x.shape[-1]
    M = x.numel() // C
    return M >= XIN_MIN_ROWS and _lib.call_int("csk_xin_qkv_ok", M, C, M // B, groups) == 1


def xin_qkv(x, stat, gamma, beta, w, bi, colsum, bq, eps):
    """(h, qkv) = (proj_in(GroupNorm(x)), LayerNorm1(h) Wqkv^T + b) in ONE
    kernel; weights / tables from ``ops.pack_xin_qkv``, ``stat`` from
    ``gn_stats``.  Returns h [M, C] and qkv [M, 3C] (bf16)."""
    _bf16(x, "xin.x")
    _bf16(w, "xin.w")
    _bf16(gamma, "xin.gamma")
    B, C = x.shape[0], x.shape[-1]
    M = x.numel() // C
    x2 = x.reshape(M, C)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    for t, n in ((bi, "bi"), (colsum, "colsum"), (bq, "bq"), (stat, "stat")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"xin_qkv: {n} must be contiguous fp32")
    if beta is not None:
        _bf16(beta, "xin.beta")
    h = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    qkv = torch.empty((M, 3 * C), dtype=torch.bfloat16, device=x.device)
    _lib.call("csk_xin_qkv", _p(h), _p(qkv), _p(x2), _p(stat), _p(gamma.contiguous()),
              _p(None if beta is None else beta.contiguous()), stat.shape[1], _p(w.contiguous()), _p(bi), _p(colsum),
              _p(bq), M, M // B, float(eps), _s())
    return h, qkv


# ---------------------------------------------------------------------------
# KV-cached decode: skinny-M GEMV (csrc/kernels/gemv.hip) and single-query
# split-KV attention with the K/V append fused in (csrc/kernels/attn_decode.hip).
# Called only where decode code asks for them (ops.gemv / ops.decode_attention):
# ops.gemm / ops.attention dispatch as before.  CSK_DECODE=0 / set_decode(False):
# both ops take their fallback (layer_norm / RMSNorm + gemm; index_copy_ x2 + attention).
# ---------------------------------------------------------------------------
sig("csk_gemv", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
    c_int, c_int, c_int, c_int, c_float, c_void_p)
sig("csk_gemv_ex", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p)
sig("csk_gemv_plan", c_int)
sig("csk_set_gemv_nt", c_int)
sig("csk_attention_decode", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64),
    c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p)
sig("csk_attention_decode_ex", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64),
    c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p)
sig("csk_attention_decode_ex2", c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64),
    c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
    c_int, c_void_p)
sig("csk_attn_decode_split")
DECODE = os.environ.get("CSK_DECODE", "1") == "1"
# kernel launches per op (tests assert the kernels ran)
DECODE_STATS = {"gemv": 0, "decode_attention": 0, "gemv_glu": 0}
GEMV_NORM_NONE, GEMV_NORM_LN, GEMV_NORM_RMS = 0, 1, 2  # gemv.hip GV_NORM_*
GEMV_MAX_M = 8             # gemv.hip GV_MAX_M
GEMV_LDS_FLOATS = 32768    # gemv.hip GV_LDS_FLOATS: padded rows x K fp32 the kernel keeps in LDS
DECODE_SPLIT = 64          # attn_decode.hip AD_SPLIT: keys per workgroup
DECODE_HEAD_DIMS = (32, 64, 80, 128)  # 80 (OPT-2.7B) without rope=
_DECODE_WS: dict = {}      # (device, B, H, S, D) -> (fp32 partials, uint32 counters)


def set_decode(on: bool):
    """Decode kernels on / off (off: ``gemv`` and ``decode_attention`` take their
    fallbacks).  Read at launch: a hipGraph captured before the call keeps the
    kernels it was captured with (Bark: drop ``model._graph``)."""
    global DECODE
    DECODE = bool(on)


def set_gemv_nt(on: bool):
    """Non-temporal (default) or default-policy weight loads of the GEMV: the
    A/B knob of tools/decodebench.py."""
    _lib.call("csk_set_gemv_nt", int(bool(on)))


def _aligned_rows(t, single_row_ok=False):
    """t [R, C]: last dim contiguous, 16-byte aligned base and rows"""
    return (t.stride(1) == 1 and t.data_ptr() % 16 == 0
            and (t.stride(0) % 8 == 0 or (single_row_ok and t.shape[0] == 1)))


def rms_norm(x, gamma, eps):
    """RMSNorm of the last dim in torch (fp32 inside, rounded to x's dtype): the
    fallback of the GEMV's ``rms=`` prologue."""
    from . import _ref_rms_norm

    return _ref_rms_norm(x, gamma, eps).to(x.dtype)


def _gemv_kernel_takes(M, K):
    mt = 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8
    return DECODE and 1 <= M <= GEMV_MAX_M and K % 8 == 0 and K >= 8 and mt * K <= GEMV_LDS_FLOATS


def _gemv_norm(ln, rms, K):
    """(mode, gamma, beta, eps) of the kernel's prologue"""
    if ln is None and rms is None:
        return GEMV_NORM_NONE, None, None, 0.0
    if ln is not None:
        mode, (gamma, beta, eps), what = GEMV_NORM_LN, ln, "LayerNorm"
    else:
        mode, (gamma, eps), beta, what = GEMV_NORM_RMS, rms, None, "RMSNorm"
    _bf16(gamma, "gemv.gamma")
    if gamma.numel() != K or (beta is not None and beta.numel() != K):
        raise ValueError(f"gemv: {what} affine of {gamma.numel()} elements for K = {K}")
    gamma = gamma.contiguous()
    if gamma.data_ptr() % 16:
        gamma = gamma.clone()
    if beta is not None:
        _bf16(beta, "gemv.beta")
        beta = beta.contiguous()
        if beta.data_ptr() % 16:
            beta = beta.clone()
    return mode, gamma, beta, float(eps)


def gemv(x2, w, bias=None, act=None, residual=None, ln=None, out=None, rms=None):
    """y[M, N] = act(norm?(x2)[M, K] @ w[N, K]^T + bias) + residual on the GEMV
    kernel for M <= 8; ``ln = (gamma, beta, eps)`` or ``rms = (gamma, eps)``.
    ``x2``, ``residual`` and ``out`` may be row-strided views, ``w`` a view whose
    row stride is a multiple of 8.  What the kernel does not take (M > 8, K % 8,
    GEGLU, rows beyond its LDS budget) runs layer_norm / RMSNorm + gemm instead."""
    _bf16(x2, "gemv.x")
    _bf16(w, "gemv.w")
    M, K = x2.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemv: K mismatch {tuple(x2.shape)} x {tuple(w.shape)}")
    code = ACT[act]
    if not _gemv_kernel_takes(M, K) or code == 3:
        if ln is not None:
            x2 = layer_norm(x2, ln[0], ln[1], ln[2])
        elif rms is not None:
            x2 = rms_norm(x2, rms[0], rms[1])
        y = gemm(x2, w, bias, residual, act, out=out if out is not None and out.is_contiguous() else None)
        if out is not None and y is not out:
            out.copy_(y)
            return out
        return y
    if not _aligned_rows(x2, single_row_ok=True):
        x2 = x2.contiguous()
    if not _aligned_rows(w):
        w = w.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x2.device)
    elif out.shape != (M, N) or out.dtype != torch.bfloat16 or out.stride(1) != 1 or out.device != x2.device:
        raise ValueError(f"gemv: out must be a bf16 [{M}, {N}] view with a contiguous last dim")
    ldr = 0
    if residual is not None:
        _bf16(residual, "gemv.residual")
        residual = residual.reshape(M, N)
        if residual.stride(1) != 1:
            residual = residual.contiguous()
        ldr = residual.stride(0)
    if bias is not None:
        _bf16(bias, "gemv.bias")
        bias = bias.contiguous()
    mode, gamma, beta, eps = _gemv_norm(ln, rms, K)
    _lib.call("csk_gemv_ex", _p(out), _p(x2), _p(w), None, _p(bias), _p(residual), _p(gamma), _p(beta), mode, M, N, K,
              x2.stride(0), w.stride(0), 0, ldr, out.stride(0), code, eps, _s())
    DECODE_STATS["gemv"] += 1
    return out


def gemv_glu(x2, wg, wu, act="silu", rms=None, ln=None, out=None):
    """y[M, N] = act(x' @ wg[N, K]^T) * (x' @ wu[N, K]^T), x' = norm?(x2), on the
    gated GEMV kernel for M <= 8: both matrices are streamed where they lie (views
    with a row stride that is a multiple of 8 are fine).  Outside the kernel's
    limits: the norm, two ``gemm`` calls and a multiply."""
    _bf16(x2, "gemv_glu.x")
    _bf16(wg, "gemv_glu.w_gate")
    _bf16(wu, "gemv_glu.w_up")
    M, K = x2.shape
    N = wg.shape[0]
    if wg.shape != wu.shape or wg.shape[1] != K:
        raise ValueError(f"gemv_glu: shapes {tuple(x2.shape)} x {tuple(wg.shape)} / {tuple(wu.shape)}")
    code = ACT[act]
    if code == 3:
        raise ValueError("gemv_glu: act is the gate's pointwise activation, not 'geglu'")
    if out is not None and (out.shape != (M, N) or out.dtype != torch.bfloat16 or out.stride(1) != 1
                            or out.device != x2.device):
        raise ValueError(f"gemv_glu: out must be a bf16 [{M}, {N}] view with a contiguous last dim")
    if not _gemv_kernel_takes(M, K):
        if ln is not None:
            x2 = layer_norm(x2, ln[0], ln[1], ln[2])
        elif rms is not None:
            x2 = rms_norm(x2, rms[0], rms[1])
        y = gemm(x2, wg, None, None, act) * gemm(x2, wu, None, None, None)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if not _aligned_rows(x2, single_row_ok=True):
        x2 = x2.contiguous()
    if not _aligned_rows(wg):
        wg = wg.contiguous()
    if not _aligned_rows(wu):
        wu = wu.contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x2.device)
    mode, gamma, beta, eps = _gemv_norm(ln, rms, K)
    _lib.call("csk_gemv_ex", _p(out), _p(x2), _p(wg), _p(wu), None, None, _p(gamma), _p(beta), mode, M, N, K,
              x2.stride(0), wg.stride(0), wu.stride(0), 0, out.stride(0), code, eps, _s())
    DECODE_STATS["gemv_glu"] += 1
    return out


def gemv_plan(N):
    """(columns per wave, waves per workgroup) the GEMV launcher picks for N
    output columns, plain or gated, on the current device."""
    v = _lib.call_int("csk_gemv_plan", int(N))
    return v // 16, v % 16


def _decode_ws(device, B, H, S, D):
    """Partials and arrival counters of the split-KV decode attention, allocated
    once per (device, shape) and zeroed at allocation (the kernel leaves the
    counters at zero).  Launches that share them must be stream-ordered."""
    key = (device, B, H, S, D)
    ws = _DECODE_WS.get(key)
    if ws is None:
        nsplit = -(-S // DECODE_SPLIT)
        ws = (torch.zeros(B * H * nsplit * (D + 2), dtype=torch.float32, device=device),
              torch.zeros(B * H, dtype=torch.int32, device=device))
        _DECODE_WS[key] = ws
    return ws


def decode_attention(q, kc, vc, scale, kv_len, k_new=None, v_new=None, pos=None, rope=None, rel_bias=None):
    """``ops.decode_attention`` on the HIP path (arguments validated there).
    ``pos``: the caller's long [1] device tensor holding kv_len - 1, used by the
    fallback's index_copy_ instead of deriving it from ``kv_len``.
    The kernel takes D in ``DECODE_HEAD_DIMS`` (80 only without ``rope``);
    ``rel_bias`` (fp32 [H, P >= S]) travels to it as a pointer.  The fallback
    gathers the [H, 1, S] bias of the query's position on the device and runs
    ``attention(bias=, kv_lens=)``: no host read either way."""
    for t, n in ((q, "q"), (kc, "k_cache"), (vc, "v_cache"), (k_new, "k_new"), (v_new, "v_new")):
        if t is not None:
            _bf16(t, "decode_attention." + n)
            if t.stride(-1) != 1:
                raise ValueError("decode_attention: last dim must be contiguous")
    B, _, H, D = q.shape
    S, Hkv = kc.shape[1], kc.shape[2]
    cos = sin = None
    if rope is not None:
        cos, sin = rope
        for t in (cos, sin):
            if t.dtype != torch.float32 or t.device != q.device or t.dim() != 2 or t.shape[1] != D // 2 \
                    or t.shape[0] < S or not t.is_contiguous():
                raise ValueError(f"decode_attention: rope tables must be contiguous fp32 [P >= {S}, {D // 2}] on "
                                 f"the device of q, got {tuple(t.shape)} {t.dtype}")

    def vec_ok(t):
        return t is None or (t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:3]))

    if (not DECODE or D not in DECODE_HEAD_DIMS or B * H > 65535 or not (vec_ok(kc) and vec_ok(vc))
            or (cos is not None and (D == 80 or cos.data_ptr() % 16 or sin.data_ptr() % 16))
            or (rel_bias is not None and rel_bias.data_ptr() % 16)):
        if (k_new is not None or rope is not None) and pos is None:
            pos = (kv_len.to(torch.long) - 1).clamp_(0, S - 1)
        if rope is not None:
            from . import _ref_rope

            c, s = cos.index_select(0, pos), sin.index_select(0, pos)  # [1, D / 2]
            q = _ref_rope(q, c, s).to(q.dtype)
            if k_new is not None:
                k_new = _ref_rope(k_new, c, s).to(k_new.dtype)
        if k_new is not None:
            kc.index_copy_(1, pos, k_new)
            vc.index_copy_(1, pos, v_new)
        if Hkv != H:  # (a copy: this path is for correctness, not speed)
            kc, vc = (t[:, :, :, None].expand(B, S, Hkv, H // Hkv, D).reshape(B, S, H, D) for t in (kc, vc))
        if rel_bias is not None:  # key j sits at distance kv_len - 1 - j (keys at or past kv_len: masked by kv_lens)
            dist = (kv_len.to(torch.long) - 1 - torch.arange(S, device=q.device)).clamp_(0, rel_bias.shape[1] - 1)
            return attention_bias(q, kc, vc, scale, False, rel_bias.index_select(1, dist)[:, None],
                                  kv_len.clamp(0, S).expand(B).contiguous())
        return attention(q, kc, vc, scale, kv_len=kv_len)
    if not vec_ok(q):
        q = q.contiguous()
    if not vec_ok(k_new):
        k_new = k_new.contiguous()
    if not vec_ok(v_new):
        v_new = v_new.contiguous()
    o = torch.empty((B, 1, H, D), dtype=torch.bfloat16, device=q.device)
    ws, cnt = _decode_ws(q.device, B, H, S, D)

    def bh(t):
        return (t.stride(0), t.stride(2)) if t is not None else (0, 0)

    st = (c_int64 * 14)(*bh(q), *kc.stride()[:3], *vc.stride()[:3], *bh(k_new), *bh(v_new), *bh(o))
    _lib.call("csk_attention_decode_ex2", _p(o), _p(q), _p(kc), _p(vc), _p(k_new), _p(v_new), st, B, H, Hkv, S, D,
              float(scale), _p(kv_len), _p(ws), _p(cnt), _p(cos), _p(sin), 0 if cos is None else cos.shape[0],
              _p(rel_bias), 0 if rel_bias is None else rel_bias.shape[1], _s())
    DECODE_STATS["decode_attention"] += 1
    return o
