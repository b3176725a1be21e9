#!/usr/bin/env python
"""Same-process, alternating A/B of the KV-cached decode path: the skinny-M GEMV
(``ops.gemv``, csrc/kernels/gemv.hip) and the single-query split-KV attention
with the fused append (``ops.decode_attention``, csrc/kernels/attn_decode.hip)
against what ran before them (``layer_norm`` + MFMA ``gemm``; ``index_copy_`` x2 +
``attention(kv_len=)``).

    python tools/decodebench.py [--rounds 7] [--only step,gemv,attn] [--out profiles/decode_<tag>.txt]

  step-<kv_len>       one whole decode step of the Bark-large semantic GPT (24 layers, C = 1024, 16 heads, the
                      10048-row head) at kv_len = 257 / 512 / 1000.  THE arm that counts: the step's ~620 MB of
                      weights are the real working set, far past the 256 MB last-level cache.
                      "off" = set_decode(False), what the parent commit launched (9 launches per layer);
                      "on" = the new kernels (5 per layer); "on-nt0" = the same with default-policy weight loads
                      instead of non-temporal ones (the load-policy A/B).
  gemv-<N>x<K>        one M = 1 projection, old (gemm) against new (gemv, gemv-nt0), rotating through 24 distinct
                      weight buffers per graph so that no call finds its matrix in a cache a real step would have
                      flushed (a single matrix replayed alone flatters every kernel).
  attn-<kv_len>       H = 16, D = 64, S = 1024: index_copy_ x2 + attention against decode_attention with the
                      append, rotating through 24 caches.

"copy": ``dst.copy_(src)`` moving the same bytes (half read, half written), the bandwidth yardstick of the box.
Every arm is a captured hipGraph replayed between device events; the arms alternate within a round and the median
[min .. max] over the rounds is reported as us per call (per step) and achieved GB/s, with the bytes computed
here from the shapes: weights (+ bias) + the live K/V rows; activations are noise beside them.
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chiaswarm_amd import ops  # noqa: E402
from chiaswarm_amd.ops import _lib, hip_ops  # noqa: E402

DEV = "cuda"
NBUF = 24


def capture(fn, reps=1):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(g, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / calls  # us per call


def copy_arm(nbytes, nbuf=1):
    """nbuf copies of nbytes each (half read, half written), from rotating sources"""
    srcs = [torch.randn(max(nbytes // 4, 8), device=DEV).bfloat16() for _ in range(nbuf)]
    dst = torch.empty_like(srcs[0])

    def fn():
        for s in srcs:
            dst.copy_(s)
    return fn


def with_switch(on, nt, make):
    """build + capture an arm under a decode switch / load policy (both are read at launch, so the captured
    graph keeps them)"""
    hip_ops.set_decode(on)
    hip_ops.set_gemv_nt(nt)
    try:
        return make()
    finally:
        hip_ops.set_decode(True)
        hip_ops.set_gemv_nt(True)


def run_case(say, name, nbytes, graphs, calls, rounds, base, note=""):
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            t[k].append(timed(g, calls))
    med = {k: statistics.median(v) for k, v in t.items()}
    say(f"{name}  ({nbytes / 1e6:.2f} MB per call){note}")
    for k in graphs:
        extra = "" if k in (base, "copy") else f"   {base}/this {med[base] / med[k]:5.2f}x"
        if k not in (base, "copy") and min(t[base]) > max(t[k]):
            extra += "  (ranges disjoint)"
        elif k not in (base, "copy"):
            extra += "  (ranges overlap)"
        say(f"  {k:8s}{med[k]:9.1f} us [{min(t[k]):8.1f} .. {max(t[k]):8.1f}]  {nbytes / med[k] / 1e3:7.0f} GB/s{extra}")
    return med


@torch.no_grad()
def step_cases(say, rounds, lens, steps_per_graph):
    from chiaswarm_amd.models import bark as bk
    from chiaswarm_amd.models.layers import init_random_fast_, prepare_model

    sc, _, _ = bk.bark_configs("large")
    with torch.device(DEV):
        m = bk.BarkCausalGPT(sc).to(torch.bfloat16).eval().requires_grad_(False)
    init_random_fast_(m, seed=1)
    prepare_model(m)
    m.new_cache()
    C, L, H = sc.n_embd, sc.n_layer, sc.n_head
    for kc, vc in m.cache:
        kc.normal_()
        vc.normal_()
    ids = torch.full((1, 1), 17, dtype=torch.long, device=DEV)
    wbytes = L * 12 * C * C * 2 + sc.out_vocab * C * 2
    for n in lens:
        pos_t = torch.tensor([n - 1], device=DEV)
        len_t = torch.tensor([n], dtype=torch.int32, device=DEV)
        nbytes = wbytes + L * 2 * n * C * 2
        outs = {}

        def make(key):
            def fn():
                outs[key] = m._decode_fn(ids, pos_t, len_t)
            return lambda: capture(fn, steps_per_graph)

        graphs = {"off": with_switch(False, True, make("off")), "on": with_switch(True, True, make("on")),
                  "on-nt0": with_switch(True, False, make("on-nt0")),
                  "copy": capture(copy_arm(nbytes))}
        torch.cuda.synchronize()
        err = ((outs["on"].double() - outs["off"].double()).norm() / outs["off"].double().norm()).item()
        calls = {k: steps_per_graph for k in graphs}
        calls["copy"] = 1
        # the copy graph holds one copy, the others steps_per_graph steps: time them per call
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        t = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                t[k].append(timed(g, calls[k]))
        med = {k: statistics.median(v) for k, v in t.items()}
        say(f"step-{n}  ({nbytes / 1e6:.1f} MB of weights + live K/V per step; logits on vs off rel diff {err:.1e})")
        for k in graphs:
            extra = ""
            if k not in ("off", "copy"):
                extra = f"   off/this {med['off'] / med[k]:5.2f}x  " + \
                        ("(ranges disjoint)" if min(t["off"]) > max(t[k]) else "(ranges overlap)")
            say(f"  {k:8s}{med[k]:9.1f} us [{min(t[k]):8.1f} .. {max(t[k]):8.1f}]  {nbytes / med[k] / 1e3:7.0f} GB/s{extra}")
        del graphs


def gemv_cases(say, rounds):
    for N, K in ((3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (10048, 1024)):
        ws = [(torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16() for _ in range(NBUF)]
        x = (2 * torch.randn(1, K, device=DEV) + 0.5).bfloat16()
        nbytes = N * K * 2

        def old():
            for w in ws:
                hip_ops.gemm(x, w)

        def new():
            for w in ws:
                hip_ops.gemv(x, w)

        graphs = {"gemm": capture(old), "gemv": with_switch(True, True, lambda: capture(new)),
                  "gemv-nt0": with_switch(True, False, lambda: capture(new)), "copy": capture(copy_arm(nbytes, NBUF))}
        ref = x.double() @ ws[0].double().t()
        err = ((hip_ops.gemv(x, ws[0]).double() - ref).norm() / ref.norm()).item()
        run_case(say, f"gemv-{N}x{K}", nbytes, graphs, NBUF, rounds, "gemm", f"  gemv rel err vs fp64 {err:.1e}")
        del graphs, ws


def attn_cases(say, rounds, lens):
    B, H, D, S = 1, 16, 64, 1024
    scale = 1.0 / math.sqrt(D)
    caches = [(torch.randn(B, S, H, D, device=DEV).bfloat16(), torch.randn(B, S, H, D, device=DEV).bfloat16())
              for _ in range(NBUF)]
    qkv = torch.randn(B, 1, 3, H, D, device=DEV).bfloat16()
    q, kn, vn = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    for n in lens:
        pos_t = torch.tensor([n - 1], device=DEV)
        len_t = torch.tensor([n], dtype=torch.int32, device=DEV)
        nbytes = 2 * n * H * D * 2

        def old():
            for kc, vc in caches:
                kc.index_copy_(1, pos_t, kn)
                vc.index_copy_(1, pos_t, vn)
                hip_ops.attention(q, kc, vc, scale, kv_len=len_t)

        def new():
            for kc, vc in caches:
                ops.decode_attention(q, kc, vc, scale, len_t, k_new=kn, v_new=vn)

        graphs = {"old": capture(old), "new": capture(new), "copy": capture(copy_arm(nbytes, NBUF))}
        a = hip_ops.attention(q, *caches[0], scale, kv_len=len_t).double()
        err = ((ops.decode_attention(q, *caches[0], scale, len_t).double() - a).norm() / a.norm()).item()
        run_case(say, f"attn-{n}", nbytes, graphs, NBUF, rounds, "old", f"  new vs old rel diff {err:.1e}")
        del graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4, help="decode steps per captured graph of the step arm")
    ap.add_argument("--only", default="", help="comma-separated: step, gemv, attn")
    ap.add_argument("--out", default="", help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decodebench: needs the GPU (a CPU run measures nothing)")
    _lib.load()
    torch.manual_seed(0)
    only = [c for c in a.only.split(",") if c] or ["step", "gemv", "attn"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; {a.rounds} alternating rounds; us per call median [min .. max], "
        "GB/s = bytes from the shapes / median")
    if "step" in only:
        step_cases(say, a.rounds, (257, 512, 1000), a.steps)
    if "gemv" in only:
        gemv_cases(say, a.rounds)
    if "attn" in only:
        attn_cases(say, a.rounds, (257, 1000))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
