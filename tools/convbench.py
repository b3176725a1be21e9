#!/usr/bin/env python
"""One implicit-GEMM conv (or plain GEMM) shape in a loop, fixed tile / split,
for PMC counter runs and tile A/Bs:

    python tools/convbench.py --shape 8,64,64,320,320 --tiles 11,19,25 --iters 50
    python tools/convbench.py --gemm 32768,1280,320 --tiles 11,25
    python tools/convbench.py --shortcut [--batch 8]   # fused conv2 vs conv2 + shortcut GEMMs, the 14 SD2.1 sites
    rocprofv3 --kernel-trace --pmc SQ_INSTS_MFMA ... -- python3 tools/convbench.py --tiles 11 --iters 5
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chiaswarm_amd import ops  # noqa: E402
from chiaswarm_amd.ops import _lib  # noqa: E402
from chiaswarm_amd.ops.hip_ops import _p, _s  # noqa: E402


# SD2.1 ResNets with a 1x1 shortcut at 64x64 latents: (H = W, shortcut sources, Cout); 2 down, 12 up
SD21_SHORTCUTS = [(32, (320,), 640), (16, (640,), 1280),
                  (8, (1280, 1280), 1280), (8, (1280, 1280), 1280), (8, (1280, 1280), 1280),
                  (16, (1280, 1280), 1280), (16, (1280, 1280), 1280), (16, (1280, 640), 1280),
                  (32, (1280, 640), 640), (32, (640, 640), 640), (32, (640, 320), 640),
                  (64, (640, 320), 320), (64, (320, 320), 320), (64, (320, 320), 320)]


def _graph_us(fn, iters):
    """device time of fn() per call: iters calls captured in one hipGraph, replayed"""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1000)
    return sorted(ts)[len(ts) // 2]


def shortcut_bench(batch, iters):
    """conv2 with the shortcut as extra K segments against conv2 (shortcut as its
    residual) + the shortcut GEMM(s), each with its tuned plan, per distinct site"""
    from chiaswarm_amd.ops import hip_ops

    dev = "cuda"
    seen, tot_u, tot_f = {}, 0.0, 0.0
    for H, srcs, cout in SD21_SHORTCUTS:
        key = (H, srcs, cout)
        if key not in seen:
            r = lambda *sh, sc=1.0: (torch.randn(*sh, device=dev) * sc).bfloat16()  # noqa: E731
            h = r(batch, H, H, cout)
            xs = [r(batch, H, H, c) for c in srcs]
            K = 9 * cout + sum(srcs)
            wp = ops.pack_conv_weight(r(cout, cout, 3, 3, sc=K ** -0.5))
            wsc = r(cout, sum(srcs), sc=K ** -0.5)
            bias = r(cout)
            _, wv, (wf,) = ops.pack_conv_extra(wp, [wsc])
            extra, off = [], 0
            for t, c in zip(xs, srcs):
                extra.append((t, wf[:, off:off + c]))
                off += c
            extra = tuple(extra)

            def unfused():
                sc = hip_ops.gemm(xs[0].view(-1, srcs[0]), wsc[:, :srcs[0]], bias if len(xs) == 1 else None)
                if len(xs) > 1:
                    sc = hip_ops.gemm(xs[1].view(-1, srcs[1]), wsc[:, srcs[0]:], bias, residual=sc)
                return hip_ops.conv2d(h, wp, bias, 1, 1, sc.view(batch, H, H, cout), False, None, gn_stats=True)

            def fused():
                return hip_ops.conv2d(h, wv, bias, 1, 1, None, False, None, gn_stats=True, extra=extra)

            seen[key] = (_graph_us(unfused, iters), _graph_us(fused, iters))
        u, f = seen[key]
        tot_u += u
        tot_f += f
    for (H, srcs, cout), (u, f) in seen.items():
        n = sum(1 for s in SD21_SHORTCUTS if s == (H, srcs, cout))
        print(f"{n} x {H:2d}x{H:<2d} conv2 {cout:4d} + shortcut {'|'.join(map(str, srcs)):9s}: conv2 + GEMMs {u:7.1f} us  "
              f"fused {f:7.1f} us  ({f - u:+6.1f})", flush=True)
    print(f"per step (14 sites, batch {batch}): conv2 + GEMMs {tot_u:7.1f} us  fused {tot_f:7.1f} us  "
          f"({tot_f - tot_u:+6.1f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="8,64,64,320,320", help="B,H,W,Cin,Cout (3x3, pad 1)")
    ap.add_argument("--gemm", default="", help="M,N,K (plain GEMM instead of the conv)")
    ap.add_argument("--tiles", default="11")
    ap.add_argument("--split", type=int, default=1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--act", type=int, default=0, help="GEMM epilogue activation code (3 = GEGLU, N = 2 x out)")
    ap.add_argument("--shortcut", action="store_true",
                    help="the 14 SD2.1 ResNet shortcut sites: conv2 with extra K segments vs conv2 + shortcut GEMMs")
    ap.add_argument("--batch", type=int, default=8, help="--shortcut: UNet batch (CFG: 2 x images)")
    a = ap.parse_args()
    _lib.load()
    dev = "cuda"
    if a.shortcut:
        return shortcut_bench(a.batch, a.iters)
    if a.gemm:
        M, N, K = map(int, a.gemm.split(","))
        x = torch.randn(M, K, device=dev).bfloat16()
        w = (torch.randn(N, K, device=dev) * K ** -0.5).bfloat16()
        No = N // 2 if a.act == 3 else N
        y = torch.empty(M, No, dtype=torch.bfloat16, device=dev)
        flops = 2 * M * N * K
        ws = torch.empty(a.split * M * N, dtype=torch.float32, device=dev)

        def run(tile):
            _lib.call("csk_gemm", _p(y), _p(x), _p(w), None, None, None, M, N, K, K, K, No, No, 1, a.act, 1.0, None,
                      tile, a.split, _p(ws), _s())

        def ref():
            r = x.float() @ w.float().t()
            if a.act == 3:  # packed (hidden, gate) 16-column pairs
                r = r.view(M, N // 32, 2, 16)
                r = (r[:, :, 0] * torch.nn.functional.gelu(r[:, :, 1])).reshape(M, No)
            return r
    else:
        B, H, W, Cin, Cout = map(int, a.shape.split(","))
        x = torch.randn(B, H, W, Cin, device=dev).bfloat16()
        wp = ops.pack_conv_weight((torch.randn(Cout, Cin, 3, 3, device=dev) * (9 * Cin) ** -0.5).bfloat16())
        y = torch.empty(B, H, W, Cout, dtype=torch.bfloat16, device=dev)
        flops = 2 * B * H * W * Cout * Cin * 9
        ws = torch.empty(a.split * B * H * W * Cout, dtype=torch.float32, device=dev)

        def run(tile):
            _lib.call("csk_conv2d", _p(y), _p(x), _p(wp), None, None, None, B, H, W, Cin, Cout, 3, 3, 1, 1, 1, H, W, 0,
                      Cin, Cout, 0, 0, 1.0, 1, None, tile, a.split, _p(ws), _s())

        def ref():
            return ops._ref_conv2d(x.float(), wp.float(), None, 1, 1, None, False, None)
    for tile in map(int, a.tiles.split(",")):
        for _ in range(3):
            run(tile)
        torch.cuda.synchronize()
        if a.check:
            r = ref()
            err = ((y.float() - r).norm() / r.norm()).item()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run(tile)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        extra = f"  rel_err {err:.2e}" if a.check else ""
        print(f"tile {tile:2d} split {a.split}: {ms * 1000:8.1f} us  {flops / ms / 1e9:7.1f} TF/s{extra}", flush=True)


if __name__ == "__main__":
    main()
