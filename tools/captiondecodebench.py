#!/usr/bin/env python
"""Time per generated token of BLIP-2's two language models, OPT-2.7B
(``models/blip2.py``) and Flan-T5-XL (``models/t5.py``): the sequence re-run
that greedy decode did before the KV cache against the cached one-token step,
in one process, alternating.

    python tools/captiondecodebench.py [--rounds 9] [--layers 0] [--out profiles/caption_decode_<tag>.txt]

Language-model geometry only (OPT: 32 layers, dim 2560, 32 heads of 80, ffn 10240, vocab 50272; Flan-T5-XL decoder:
24 layers, d_model 2048, 32 heads of 64, d_ff 5120, vocab 32128), random-init bf16; the vision tower and the Q-Former
are not built.  A 32-row image-query prefix plus a 16-token prompt: OPT's sequence is [prefix; prompt; generated],
T5's encoder output has 48 rows and its decoder holds the start token and the generated ones.  At g = 1 / 8 / 20
tokens already generated, the time to produce the next token:

  rerun    OPT ``text_logits`` over the whole sequence, T5 ``decode_logits`` over the decoder prefix (with every
           layer's cross-attention K/V projected again), eager: what ``generate`` ran per token before the cache, and
           still runs with ``use_cache=False`` (the yardstick)
  eager    ``decode_step``'s work launched eagerly: the state writes and ``_decode_fn``
  graph    ``decode_step``: the state writes and one hipGraph replay

Each arm is timed with a host clock around the call and the ``int(logits.argmax())`` that ends every decode iteration
(a device synchronise), after a warm-up of every shape and one discarded alternating round; the arms alternate within
a round and the median [min .. max] over the rounds is reported in ms per token.  GB/s = the step's weight bytes
(computed here from the shapes; the live K/V rows and activations are under 1 % of them) over the median.  The cached
logits are compared with the re-run's on the same sequence at every length.

Verdict (the project's A/B rule): the cached path is a model's default only if at every measured length
median(rerun) - median(graph) >= 3 x the larger of the two arms' spreads (max - min over the rounds).

Last, the decode attention alone at OPT-2.7B's shape (H = 32, D = 80, capacity 256, the append fused in): the D = 80
kernel against the fallback it replaces (``set_decode(False)``: index_copy_ x2 + ``attention(kv_len=)``), 200 calls per
sample, alternating, us per call.
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chiaswarm_amd import ops  # noqa: E402
from chiaswarm_amd.models.blip2 import BLIP2_FLAN_T5_XL, BLIP2_OPT_2_7B, Blip2Captioner  # noqa: E402
from chiaswarm_amd.models.layers import init_random_fast_, prepare_model  # noqa: E402
from chiaswarm_amd.models.t5 import T5Seq2Seq  # noqa: E402
from chiaswarm_amd.ops import _lib, hip_ops  # noqa: E402
from chiaswarm_amd.pipelines.graphs import graphs_enabled  # noqa: E402

DEV = "cuda"
PREFIX, PROMPT = 32, 16
GENERATED = (1, 8, 20)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tok = int(fn().argmax())  # the host read that ends a decode iteration: a device synchronise
    return (time.perf_counter() - t0) * 1e3, tok


def ab(say, name, wbytes, rounds, arms_at):
    """``arms_at(g)`` -> {"rerun": fn, "eager": fn, "graph": fn}; returns the verdict"""
    ok = True
    for g in GENERATED:
        arms = arms_at(g)
        outs = {}
        for k, fn in arms.items():  # warm-up of every shape (tile choices, the graph capture), and the outputs
            for _ in range(2):
                outs[k] = fn().double().clone()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        toks = {}
        for r in range(rounds + 1):  # the first alternating round is part of the warm-up (the allocator settles)
            for k, fn in arms.items():
                ms, toks[k] = timed(fn)
                if r:
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: max(v) - min(v) for k, v in t.items()}
        err = {k: ((outs[k] - outs["rerun"]).norm() / outs["rerun"].norm()).item() for k in ("eager", "graph")}
        say(f"{name} generated-{g}  (cached vs re-run logits rel diff: eager {err['eager']:.1e}, graph "
            f"{err['graph']:.1e}; next token re-run {toks['rerun']}, eager {toks['eager']}, graph {toks['graph']})")
        for k in arms:
            extra = ""
            if k in ("eager", "graph"):
                extra = f"   rerun/this {med['rerun'] / med[k]:5.2f}x"
            say(f"  {k:6s}{med[k]:9.3f} ms [{min(t[k]):8.3f} .. {max(t[k]):8.3f}]  {wbytes / med[k] / 1e6:7.0f} GB/s{extra}")
        need = 3 * max(spread["rerun"], spread["graph"])
        won = med["rerun"] - med["graph"] >= need
        ok = ok and won
        say(f"  rerun - graph = {med['rerun'] - med['graph']:.3f} ms against 3 x the larger spread = {need:.3f} ms: "
            + ("cached wins" if won else "NOT decided"))
    say(f"{name}: " + ("cached decode wins at every length: use_cache defaults to on" if ok else
                       "cached decode does NOT win at every length: use_cache must default to off"))
    return ok


def eager_launches(fn):
    before = dict(hip_ops.DECODE_STATS)
    fn()
    d = {k: hip_ops.DECODE_STATS[k] - before[k] for k in before}
    return d, sum(d.values())


@torch.no_grad()
def bench_opt(say, rounds, layers):
    cfg = dataclasses.replace(BLIP2_OPT_2_7B, image_size=28, vision_dim=32, vision_depth=1, vision_heads=2,
                              vision_mlp=64, q_dim=32, q_depth=1, q_heads=2, q_mlp=64,
                              lm_depth=layers or BLIP2_OPT_2_7B.lm_depth)
    with torch.device(DEV):
        m = Blip2Captioner(cfg).to(torch.bfloat16).eval().requires_grad_(False)
    init_random_fast_(m, seed=1)
    prepare_model(m)
    d, ffn, L = cfg.lm_dim, cfg.lm_ffn, cfg.lm_depth
    wbytes = 2 * (L * (4 * d * d + 2 * d * ffn) + cfg.vocab * d)
    gen = torch.Generator(device=DEV).manual_seed(2)
    total = PREFIX + PROMPT + max(GENERATED)
    ids = torch.randint(3, cfg.vocab, (total - PREFIX,), generator=gen, device=DEV).tolist()
    prefix = torch.randn(1, PREFIX, d, generator=gen, device=DEV).bfloat16()
    m.new_cache(total)
    m.prefill(prefix, ids)  # every position's K/V, as the steps before each measured one would have left them
    st = (torch.zeros(1, 1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV),
          torch.zeros(1, dtype=torch.int32, device=DEV))

    def arms_at(g):
        n = PREFIX + PROMPT + g  # the sequence that produces token g + 1
        tok, pos = ids[n - 1 - PREFIX], n - 1

        def eager():
            st[0].fill_(tok)
            st[1].fill_(pos)
            st[2].fill_(pos + 1)
            return m._decode_fn(*st)

        return {"rerun": lambda: m.text_logits(prefix, ids[:n - PREFIX]), "eager": eager,
                "graph": lambda: m.decode_step(tok, pos)}

    counts, launches = eager_launches(arms_at(1)["eager"])
    say(f"OPT: {L} layers, dim {d}, {cfg.lm_heads} heads of {d // cfg.lm_heads}, ffn {ffn}, vocab {cfg.vocab}; one "
        f"cached step = {launches} decode-kernel launches {counts} + the embedding gather/add, streaming "
        f"{wbytes / 1e9:.2f} GB of weights")
    ok = ab(say, "OPT", wbytes, rounds, arms_at)
    del m
    torch.cuda.empty_cache()
    return ok


@torch.no_grad()
def bench_t5(say, rounds, layers):
    cfg = BLIP2_FLAN_T5_XL
    c = dataclasses.replace(cfg.t5, layers=layers or cfg.t5.layers)
    L = layers or cfg.t5_dec_layers
    with torch.device(DEV):
        m = T5Seq2Seq(c, L).to(torch.bfloat16).eval().requires_grad_(False)
        m.encoder.block = torch.nn.ModuleList()  # the decoder alone is measured: the encoder output is random
    init_random_fast_(m, seed=1)
    for blk in m.decoder.block:  # T5 folds 1 / sqrt(d_kv) into q (its scores carry no such factor)
        for a in (blk.layer[0].SelfAttention, blk.layer[1].EncDecAttention):
            a.q.weight.mul_(c.d_kv ** -0.5)
    prepare_model(m)
    d, inner, ff = c.d_model, c.heads * c.d_kv, c.d_ff
    wbytes = 2 * (L * (6 * d * inner + 3 * d * ff) + c.vocab * d)
    gen = torch.Generator(device=DEV).manual_seed(3)
    enc = torch.randn(1, PREFIX + PROMPT, d, generator=gen, device=DEV).bfloat16()
    dec = [0] + torch.randint(3, c.vocab, (max(GENERATED),), generator=gen, device=DEV).tolist()
    m.new_cache(len(dec), enc.shape[1])
    m.begin_decode(enc)
    for i, t in enumerate(dec):  # every position's K/V, as the steps before each measured one leave them
        m.decode_step(t, i)
    st = (torch.zeros(1, 1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV),
          torch.zeros(1, dtype=torch.int32, device=DEV))

    def arms_at(g):
        tok, pos = dec[g], g  # the decoder holds the start token and g generated ones

        def eager():
            st[0].fill_(tok)
            st[1].fill_(pos)
            st[2].fill_(pos + 1)
            return m._decode_fn(*st)

        return {"rerun": lambda: m.decode_logits(enc, dec[:g + 1]), "eager": eager,
                "graph": lambda: m.decode_step(tok, pos)}

    counts, launches = eager_launches(arms_at(1)["eager"])
    say(f"Flan-T5 decoder: {L} layers, d_model {d}, {c.heads} heads of {c.d_kv}, d_ff {ff}, vocab {c.vocab}, "
        f"{enc.shape[1]} encoder rows; one cached step = {launches} decode-kernel launches {counts} + the embedding "
        f"gather, streaming {wbytes / 1e9:.2f} GB of weights (the re-run also streams {2 * L * 2 * d * inner / 1e9:.2f} "
        f"GB of cross K/V weights)")
    ok = ab(say, "T5", wbytes, rounds, arms_at)
    del m
    torch.cuda.empty_cache()
    return ok


@torch.no_grad()
def bench_d80(say, rounds):
    H, D, S, calls = 32, 80, 256, 200
    gen = torch.Generator(device=DEV).manual_seed(4)
    qkv = torch.randn(1, 1, 3, H, D, generator=gen, device=DEV).bfloat16()
    kv = torch.randn(1, S, 2, H, D, generator=gen, device=DEV).bfloat16()
    kc, vc = kv[:, :, 0], kv[:, :, 1]
    for g in GENERATED:
        n = PREFIX + PROMPT + g
        len_t = torch.tensor([n], dtype=torch.int32, device=DEV)
        pos_t = torch.tensor([n - 1], device=DEV)

        def run():
            for _ in range(calls):
                o = ops.decode_attention(qkv[:, :, 0], kc, vc, D ** -0.5, len_t, k_new=qkv[:, :, 1], v_new=qkv[:, :, 2],
                                         pos=pos_t)
            return o

        t, outs = {"kernel": [], "fallback": []}, {}
        for r in range(rounds + 1):  # the first round is the warm-up
            for k in t:
                hip_ops.set_decode(k == "kernel")
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[k] = run().double()
                    torch.cuda.synchronize()
                    if r:
                        t[k].append((time.perf_counter() - t0) * 1e6 / calls)
                finally:
                    hip_ops.set_decode(True)
        med = {k: statistics.median(v) for k, v in t.items()}
        err = ((outs["kernel"] - outs["fallback"]).norm() / outs["fallback"].norm()).item()
        say(f"decode attention H={H} D={D} capacity {S} kv_len {n} (eager launches, host-timed): kernel "
            f"{med['kernel']:.1f} us [{min(t['kernel']):.1f} .. {max(t['kernel']):.1f}], fallback {med['fallback']:.1f} us "
            f"[{min(t['fallback']):.1f} .. {max(t['fallback']):.1f}], fallback/kernel {med['fallback'] / med['kernel']:.2f}x, "
            f"rel diff {err:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers: a rehearsal, not the production geometry")
    ap.add_argument("--out", default="", help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("captiondecodebench: needs the GPU (a CPU run measures nothing)")
    _lib.load()
    if not graphs_enabled(torch.device(DEV)):
        sys.exit("captiondecodebench: the HIP path is off, there is no graph arm to time")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(0)}; bf16, random init; {PREFIX}-row prefix + {PROMPT}-token prompt; {a.rounds} "
        f"alternating rounds; ms per token median [min .. max]; GB/s = weight bytes per step / median")
    bench_opt(say, a.rounds, a.layers)
    bench_t5(say, a.rounds, a.layers)
    bench_d80(say, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
