#!/usr/bin/env python
"""The fused cross-attention sub-block (xattn.hip) on the SD2.1 64x64-level
shape, with its profiling probes (csk_set_xattn_probe: 1 no Q-projection MFMAs,
2 no attention, 4 no out-projection MFMAs, 8 no per-head DMA, 15 all) for the
4-wave and 8-wave workgroups (csk_set_xattn_waves), against
the unfused chain (LN-fused Q GEMM + attn_shortkv + out-projection GEMM):

    python tools/xattnbench.py [--batch 8] [--iters 30]
    python tools/xattnbench.py --pre [--batch 8]   # out-projection as the prologue vs out-projection GEMM + block
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chiaswarm_amd import ops  # noqa: E402
from chiaswarm_amd.models.layers import BasicTransformerBlock, init_random_fast_, prepare_model  # noqa: E402
from chiaswarm_amd.ops import _lib, hip_ops  # noqa: E402


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1000


def pre_bench(batch, hw, iters):
    """The fused block with the self-attention out-projection as its prologue
    (xattn_block(pre=...)) against the out-projection GEMM + the fused block,
    and for the CFG-shared first block (both halves from the half batch)
    against today's chain there (half-batch Q GEMM, two dup2, attn_shortkv,
    out-projection GEMM), each in one hipGraph."""
    from ffbench import graph_us

    dev = torch.device("cuda", 0)
    C = 320
    with torch.device(dev):
        blk = BasicTransformerBlock(C, C // 64, 64, 1024).to(torch.bfloat16).eval()
    init_random_fast_(blk, seed=1)
    prepare_model(blk)
    S = hw * hw
    a1, a2 = blk.attn1, blk.attn2
    kv = a2.context_kv(torch.randn(batch, 77, 1024, device=dev).bfloat16())
    f = blk._fold("q", a2.to_q.weight, a2.to_q.bias, blk.norm2)
    wqp = ops.permute_xattn_q(f[0])
    wo, bo, wo1, bo1 = a2.to_out[0].weight, a2.to_out[0].bias, a1.to_out[0].weight, a1.to_out[0].bias
    xr = ops.row_stats_wanted(kv)
    for half in (False, True):
        bs = batch // 2 if half else batch
        o = torch.randn(bs, S, C, device=dev).bfloat16()
        h0 = torch.randn(bs, S, C, device=dev).bfloat16()

        def fused():
            return hip_ops.xattn_block(None, wqp, f[1], f[2], kv, wo, bo, 1e-5, a2.scale, S, pre=(o, h0, wo1, bo1),
                                       batch=batch)

        def chain():
            x = ops.gemm(o, wo1, bo1, residual=h0, row_stats=xr)
            if not half:
                return hip_ops.xattn_block(x, *f, kv, wo, bo, 1e-5, a2.scale, S)
            q = ops.layer_norm_gemm(x, blk.norm2, a2.to_q.weight, a2.to_q.bias, f)
            return a2.attend_q(ops.dup2(q), kv, None, residual=ops.dup2(x), row_stats=True)

        t_c, t_f = graph_us(chain, iters), graph_us(fused, iters)
        err = ((fused().float() - chain().float()).norm() / chain().float().norm()).item()
        what = "CFG-shared first block (half-batch source)" if half else "out-proj GEMM + xattn block"
        print(f"B{batch} {what}: chain {t_c:6.1f} us  fused {t_f:6.1f} us  saved {t_c - t_f:5.1f} us "
              f"({t_c / t_f:.2f}x)  rel diff {err:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--pre", action="store_true",
                    help="the out-projection as the block's prologue vs the GEMM + block chain, each in one hipGraph")
    a = ap.parse_args()
    _lib.load()
    if a.pre:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        return pre_bench(a.batch, a.hw, a.iters)
    dev = torch.device("cuda", 0)
    C = 320
    with torch.device(dev):
        blk = BasicTransformerBlock(C, C // 64, 64, 1024).to(torch.bfloat16).eval()
    init_random_fast_(blk, seed=1)
    prepare_model(blk)
    S = a.hw * a.hw
    x = torch.randn(a.batch, S, C, device=dev).bfloat16()
    kv = blk.attn2.context_kv(torch.randn(a.batch, 77, 1024, device=dev).bfloat16())
    a2 = blk.attn2
    w2, colsum, b2 = blk._fold("q", a2.to_q.weight, a2.to_q.bias, blk.norm2)
    wo, bo = a2.to_out[0].weight, a2.to_out[0].bias
    fl = 2.0 * a.batch * S * C * C * 2 + 4.0 * a.batch * S * 77 * C
    ref = None
    for waves in (4, 8):
        hip_ops.XATTN_WAVES = waves  # applied by the next xattn_block call
        for probe in (0, 1, 2, 4, 8, 15):
            _lib.call("csk_set_xattn_probe", probe)
            t = timeit(lambda: hip_ops.xattn_block(x, w2, colsum, b2, kv, wo, bo, 1e-5, a2.scale, S), a.iters)
            print(f"xattn {waves} waves probe {probe:2d}: {t:7.1f} us  {fl / t / 1e6:6.1f} TF/s", flush=True)
        _lib.call("csk_set_xattn_probe", 0)
        y = hip_ops.xattn_block(x, w2, colsum, b2, kv, wo, bo, 1e-5, a2.scale, S).float()
        if ref is None:
            ref = y
        else:
            print(f"  {waves} waves vs 4 waves: max abs diff {(y - ref).abs().max().item():.3e}", flush=True)
    hip_ops.XATTN_WAVES = 4
    xr = ops.row_stats_wanted(x)
    x1 = ops.gemm(x, blk.attn1.to_out[0].weight, None, row_stats=xr)  # a producer carrying row statistics

    def chain():
        q = ops.layer_norm_gemm(x1, blk.norm2, a2.to_q.weight, a2.to_q.bias, (w2, colsum, b2))
        return a2.attend_q(q, kv, None, residual=x1, row_stats=True)

    t = timeit(chain, a.iters)
    print(f"unfused chain (Q GEMM + attn_shortkv + out GEMM): {t:7.1f} us", flush=True)


if __name__ == "__main__":
    main()
