#!/usr/bin/env python
"""Same-process, alternating A/B of the depthwise NHWC conv ops
(``ops.depthwise_conv2d`` / ``ops.depthwise_conv_transpose2d``,
csrc/kernels/dwconv.hip) against the torch chains they replace, on the shapes
that run them:

    python tools/dwconvbench.py [--iters 50] [--rounds 7] [--only kdown] [--out profiles/dwconv_<tag>.txt]

  kdown-<H>-b<B>  K-UNet KDownsample2D, 384 channels, H^2 -> (H/2)^2   (H = 128, 64; B = 1, 4)
  kup-<H>-b<B>    K-UNet KUpsample2D,   384 channels, H^2 -> (2H)^2    (H = 32, 64;  B = 1, 4)
  cnx-<H>x<C>     ConvNeXt 7x7 depthwise + bias, pad 3                 (128^2 x 96 ... 16^2 x 768)

Arms.  "old": what the parent commit ran on the same NHWC bf16 tensor: for the
K-UNet permute -> F.pad(reflect) -> grouped F.conv2d / F.conv_transpose2d ->
permute -> contiguous; for ConvNeXt the grouped nn.Conv2d on the NCHW map alone
(its two layout permutes per block are NOT charged to it).  "halo" / "direct":
the two forward variants of the new kernel; "new": the transposed gather kernel.
"copy": ``dst.copy_(src)`` of a bf16 buffer of (input + output) / 2 bytes, i.e.
the same bytes moved, as the bandwidth yardstick of the same box.

Every arm is captured into a hipGraph of ``iters`` back-to-back calls (these ops
run inside captured step graphs; eager timing would measure the host's launch
rate), replayed between device events; the arms alternate within a round and the
median [min .. max] over the rounds is reported as us per call and achieved GB/s
with bytes = input + output.  The working sets (<= 63 MB) stay cache-resident
between calls, as they do between the kernels of a real step.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from chiaswarm_amd import ops  # noqa: E402
from chiaswarm_amd.models.kunet import _binomial_kernel  # noqa: E402
from chiaswarm_amd.ops import _lib, hip_ops  # noqa: E402

DEV = "cuda"


def kdown_case(B, H, C=384):
    x = torch.randn(B, H, H, C, device=DEV).bfloat16()
    k = _binomial_kernel(C).to(DEV).bfloat16()
    wp = ops.pack_depthwise_weight(k)

    def old():
        xn = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
        return F.conv2d(xn, k, stride=2, groups=C).permute(0, 2, 3, 1).contiguous()

    def new(variant):
        return lambda: hip_ops.depthwise_conv2d(x, wp, None, 2, (1, 1, 1, 1), "reflect", None, None, (H // 2, H // 2),
                                                variant=variant)

    return {"old": old, "halo": new("halo"), "direct": new("direct")}, x.numel() * 2 + x.numel() // 4 * 2


def kup_case(B, H, C=384):
    x = torch.randn(B, H, H, C, device=DEV).bfloat16()
    k = _binomial_kernel(C, 2.0).to(DEV).bfloat16()
    wp = ops.pack_depthwise_weight(k)

    def old():
        xn = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
        return F.conv_transpose2d(xn, k, stride=2, padding=3, groups=C).permute(0, 2, 3, 1).contiguous()

    def new():
        return ops.depthwise_conv_transpose2d(x, wp, None, 1, "reflect", 3)

    return {"old": old, "new": new}, x.numel() * 2 + x.numel() * 4 * 2


def cnx_case(H, C):
    x = torch.randn(1, H, H, C, device=DEV).bfloat16()
    w = (torch.randn(C, 1, 7, 7, device=DEV) / 7).bfloat16()
    b = torch.randn(C, device=DEV).bfloat16()
    wp = ops.pack_depthwise_weight(w)
    xn = x.permute(0, 3, 1, 2).contiguous()  # the parent's blocks live in NCHW

    def old():
        return F.conv2d(xn, w, b, padding=3, groups=C)

    def new(variant):
        return lambda: hip_ops.depthwise_conv2d(x, wp, b, 1, (3, 3, 3, 3), "zeros", None, None, (H, H), variant=variant)

    arms = {"old": old, "halo": new("halo"), "direct": new("direct")}
    arms["_same"] = lambda: old().permute(0, 2, 3, 1)  # the old result in the new layout, for the difference check
    return arms, x.numel() * 2 * 2


def copy_arm(nbytes):
    src = torch.randn(nbytes // 4, device=DEV).bfloat16()
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def capture(fn, iters):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(g, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated case-name prefixes")
    ap.add_argument("--out", default="", help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dwconvbench: needs the GPU (a CPU run measures nothing)")
    _lib.load()
    torch.manual_seed(0)
    cases = {}
    for B in (1, 4):
        for H in (128, 64):
            cases[f"kdown-{H}-b{B}"] = lambda B=B, H=H: kdown_case(B, H)
        for H in (32, 64):
            cases[f"kup-{H}-b{B}"] = lambda B=B, H=H: kup_case(B, H)
    for H, C in ((128, 96), (64, 192), (32, 384), (16, 768)):
        cases[f"cnx-{H}x{C}"] = lambda H=H, C=C: cnx_case(H, C)
    only = [c for c in a.only.split(",") if c]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; graphs of {a.iters} calls, {a.rounds} alternating rounds; "
        "us per call median [min .. max], GB/s = (input + output bytes) / median")
    for name, make in cases.items():
        if only and not any(name.startswith(o) for o in only):
            continue
        arms, nbytes = make()
        same = arms.pop("_same", arms["old"])
        y0 = same().float()
        errs = {k: ((fn().float() - y0).norm() / y0.norm()).item() for k, fn in arms.items() if k != "old"}
        arms["copy"] = copy_arm(nbytes)
        graphs = {k: capture(fn, a.iters) for k, fn in arms.items()}
        for g in graphs.values():  # warm-up of the graphs themselves
            g.replay()
        torch.cuda.synchronize()
        t = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                t[k].append(timed(g, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        say(f"{name}  ({nbytes / 1e6:.2f} MB in + out)")
        for k in graphs:
            extra = "" if k in ("old", "copy") else f"   old/this {med['old'] / med[k]:5.2f}x   rel diff vs old {errs[k]:.1e}"
            say(f"  {k:7s}{med[k]:8.1f} us [{min(t[k]):7.1f} .. {max(t[k]):7.1f}]  {nbytes / med[k] / 1e3:7.0f} GB/s{extra}")
        del graphs
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
