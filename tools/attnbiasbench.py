#!/usr/bin/env python
"""Same-process, alternating A/B of the bias / key-length attention op
(``ops.attention(..., bias=, kv_lens=)``, csrc/kernels/attn_bias.hip) against
the torch formula it replaces in the text encoders, on their shapes:

    python tools/attnbiasbench.py [--iters 200] [--rounds 5] [--repeats 2] [--waves 0]

  t5-xxl      B2  H64 S77 D64   [H,S,S] bias + key padding   (DeepFloyd IF)
  flan-t5-xl  B1  H32 S40 D64   [H,S,S] bias + key padding   (BLIP-2 encoder)
  dec-self-N  B1  H32 S=N D64   causal bias with -inf        (Flan-T5 decoder step N)
  dec-cross-N B1  H32 Sq=N Skv40 key padding                 (Flan-T5 decoder step N)
  xlmr-large  B16 H16 S77 D64   mixed row lengths            (AltDiffusion CFG batch 8)

"old" is what the parent ran from the same projection outputs: the fp32 torch
matmul / masked_fill / softmax chain for T5, one flash-attention call per row
over its real keys for XLM-R (row lengths given: the host read the parent
needed per row is NOT charged to it).  Each round times ``iters`` back-to-back
calls of one arm between device events; the arms alternate; the whole A/B is
repeated ``repeats`` times so the run-to-run spread is on the page.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chiaswarm_amd import ops  # noqa: E402
from chiaswarm_amd.ops import _lib, hip_ops  # noqa: E402

DEV = "cuda"


def t5_old(q, k, v, bias, mask):
    """models/t5.py before the op: [B,S,H*D] projections -> [B,S,H*D]."""
    b, s, h, d = q.shape
    qf, kf, vf = (t.transpose(1, 2).float() for t in (q, k, v))
    scores = qf @ kf.transpose(-1, -2)
    if bias is not None:
        scores = scores + bias[None]
    if mask is not None:
        scores = scores.masked_fill(~mask[:, None, None, :], float("-inf"))
    return (torch.softmax(scores, -1) @ vf).transpose(1, 2).reshape(b, s, -1).to(q.dtype)


def t5_case(B, H, Sq, Skv, D, lens, bias_kind):
    q = torch.randn(B, Sq, H, D, device=DEV).bfloat16()
    k, v = (torch.randn(B, Skv, H, D, device=DEV).bfloat16() for _ in range(2))
    bias = None
    if bias_kind:
        bias = torch.randn(H, Sq, Skv, device=DEV)
        if bias_kind == "causal":
            bias = bias.masked_fill(torch.ones(Sq, Skv, dtype=torch.bool, device=DEV).triu(1 + Skv - Sq)[None],
                                    float("-inf"))
    mask = kl = None
    if lens is not None:
        kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        mask = torch.arange(Skv, device=DEV)[None, :] < kl[:, None]
    q = q * D ** -0.25  # T5 runs unscaled scores: keep the logits O(1)
    k = k * D ** -0.25
    return (lambda: t5_old(q, k, v, bias, mask),
            lambda: ops.attention(q, k, v, 1.0, bias=bias, kv_lens=kl).reshape(B, Sq, -1))


def xlmr_case(B, H, S, D, lens):
    qkv = torch.randn(B, S, 3, H, D, device=DEV).bfloat16()
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = D ** -0.5

    def old():
        return torch.cat([ops.attention(qkv[r:r + 1, :, 0], qkv[r:r + 1, :n, 1], qkv[r:r + 1, :n, 2], scale)
                          for r, n in enumerate(lens)], 0)

    return old, lambda: ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale, kv_lens=kl)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--waves", type=int, default=0, help="waves per workgroup of the new kernel: 0 auto, 1 / 2 / 4")
    ap.add_argument("--only", default="", help="comma-separated case names")
    a = ap.parse_args()
    _lib.load()
    hip_ops.set_attn_bias_waves(a.waves)
    torch.manual_seed(0)
    mixed = [77, 5, 12, 9, 30, 7, 21, 15, 2, 2, 2, 2, 2, 2, 2, 2]  # 8 prompts + 8 (mostly empty) negatives
    cases = {
        "t5-xxl": t5_case(2, 64, 77, 77, 64, [3, 12], "full"),  # a CFG pair: empty negative + a short prompt
        "flan-t5-xl": t5_case(1, 32, 40, 40, 64, [40], "full"),
        "xlmr-large": xlmr_case(16, 16, 77, 64, mixed),
    }
    for n in (1, 4, 8):
        cases[f"dec-self-{n}"] = t5_case(1, 32, n, n, 64, None, "causal")
        cases[f"dec-cross-{n}"] = t5_case(1, 32, n, 40, 64, [37], None)
    only = [c for c in a.only.split(",") if c]
    print(f"iters {a.iters} rounds {a.rounds} repeats {a.repeats} waves {a.waves}; us per call, median [min .. max] of the rounds")
    for name, (old, new) in cases.items():
        if only and name not in only:
            continue
        y0, y1 = old().float(), new().float()
        err = ((y0 - y1).norm() / y0.norm()).item()
        for _ in range(20):  # warm-up: lazy init, caches, clocks
            old()
            new()
        torch.cuda.synchronize()
        meds = []
        for rep in range(a.repeats):
            t_old, t_new = [], []
            for _ in range(a.rounds):
                t_old.append(timed(old, a.iters))
                t_new.append(timed(new, a.iters))
            mo, mn = statistics.median(t_old), statistics.median(t_new)
            meds.append((mo, mn))
            print(f"{name:12s} A/B {rep + 1}: old {mo:7.1f} [{min(t_old):7.1f} .. {max(t_old):7.1f}]   "
                  f"new {mn:7.1f} [{min(t_new):7.1f} .. {max(t_new):7.1f}]   old/new {mo / mn:5.2f}x")
        so = max(m[0] for m in meds) - min(m[0] for m in meds)
        sn = max(m[1] for m in meds) - min(m[1] for m in meds)
        print(f"{name:12s} spread between the A/Bs: old {so:.1f} us, new {sn:.1f} us; new vs old rel diff {err:.1e}")


if __name__ == "__main__":
    main()
