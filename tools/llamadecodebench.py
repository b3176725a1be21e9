#!/usr/bin/env python
"""Time per generated token of the Vicuna-7B language model of InstructBLIP
(``models/llama.py``): the sequence re-run that greedy decode did before the KV
cache against the cached one-token step, in one process, alternating.

    python tools/llamadecodebench.py [--rounds 9] [--layers 32] [--out profiles/llama_decode_<tag>.txt]

Vicuna-7B geometry (32 layers, dim 4096, 32 heads, ffn 11008, vocab 32000), random-init bf16, a 32-row image-query
prefix plus a 16-token prompt.  At g = 1 / 32 / 128 tokens already generated, the time to produce the next token:

  rerun    ``last_logits`` over the whole [prefix; prompt; g tokens] sequence, eager: what ``generate`` ran per
           token before the cache, and still runs with ``use_cache=False`` (the yardstick)
  eager    ``decode_step``'s work launched eagerly: the state writes and ``_decode_fn`` (5 launches a layer)
  graph    ``decode_step``: the state writes and one hipGraph replay
  copy     ``dst.copy_(src)`` moving as many bytes as a step's weights (half read, half written): what the box
           gives a plain stream of that size

Each arm is timed with a host clock around the call and the ``int(logits.argmax())`` that ends every decode
iteration (a device synchronise), after a warm-up of every shape; the arms alternate within a round and the median
[min .. max] over the rounds is reported in ms per token.  GB/s = the step's weight bytes (every layer's seven
matrices and the head, computed here from the shapes; the live K/V rows and activations are under 1 % of them) over
the median; for "rerun" the same bytes (its GEMMs stream the same weights once).  The cached logits are compared
with the re-run's on the same sequence at every length.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from chiaswarm_amd.models.layers import init_random_fast_, prepare_model  # noqa: E402
from chiaswarm_amd.models.llama import LlamaConfig, LlamaLM  # noqa: E402
from chiaswarm_amd.ops import _lib  # noqa: E402
from chiaswarm_amd.pipelines.graphs import graphs_enabled  # noqa: E402

DEV = "cuda"
PREFIX, PROMPT = 32, 16
GENERATED = (1, 32, 128)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tok = int(fn().argmax())  # the host read that ends a decode iteration: a device synchronise
    return (time.perf_counter() - t0) * 1e3, tok


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal, not Vicuna-7B")
    ap.add_argument("--out", default="", help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("llamadecodebench: needs the GPU (a CPU run measures nothing)")
    _lib.load()
    if not graphs_enabled(torch.device(DEV)):
        sys.exit("llamadecodebench: the HIP path is off, there is no graph arm to time")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    c = LlamaConfig(layers=a.layers)
    with torch.device(DEV):
        m = LlamaLM(c).to(torch.bfloat16).eval().requires_grad_(False)
    init_random_fast_(m, seed=1)
    prepare_model(m)
    hd = c.dim // c.heads
    wbytes = 2 * (c.layers * (2 * c.heads * hd * c.dim + 2 * c.kv_heads * hd * c.dim + 3 * c.dim * c.ffn)
                  + c.vocab * c.dim)
    say(f"{torch.cuda.get_device_name(0)}; LLaMA {c.layers} layers, dim {c.dim}, {c.heads} heads ({c.kv_heads} K/V), "
        f"ffn {c.ffn}, vocab {c.vocab}, bf16; {PREFIX}-row prefix + {PROMPT}-token prompt; {a.rounds} alternating "
        f"rounds; ms per token median [min .. max]; GB/s = {wbytes / 1e9:.2f} GB of weights per step / median")

    gen = torch.Generator(device=DEV).manual_seed(2)
    total = PREFIX + PROMPT + max(GENERATED)
    ids = torch.randint(3, c.vocab, (1, total - PREFIX), generator=gen, device=DEV)
    prefix = torch.randn(1, PREFIX, c.dim, generator=gen, device=DEV).bfloat16()
    x_full = torch.cat([prefix, m.model.embed_tokens(ids)], 1)
    m.new_cache(total)
    m.prefill(x_full)  # every position's K/V, as the steps before each measured one would have left them

    src = torch.empty(wbytes // 4, dtype=torch.bfloat16, device=DEV).normal_()
    dst = torch.empty_like(src)
    st = (torch.zeros(1, 1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV),
          torch.zeros(1, dtype=torch.int32, device=DEV))

    for g in GENERATED:
        n = PREFIX + PROMPT + g          # the sequence that produces token g + 1
        tok, pos = int(ids[0, n - 1 - PREFIX]), n - 1

        def rerun():
            return m.last_logits(x_full[:, :n])

        def eager():
            st[0].fill_(tok)
            st[1].fill_(pos)
            st[2].fill_(pos + 1)
            return m._decode_fn(*st)

        def graph():
            return m.decode_step(tok, pos)

        def copy():
            dst.copy_(src)
            return dst[:8]

        arms = {"rerun": rerun, "eager": eager, "graph": graph, "copy": copy}
        outs = {}
        for k, fn in arms.items():  # warm-up of every shape (tile choices, the graph capture), and the outputs
            for _ in range(2):
                outs[k] = fn().double().clone()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        toks = {}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ms, toks[k] = timed(fn)
                t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        err = {k: ((outs[k] - outs["rerun"]).norm() / outs["rerun"].norm()).item() for k in ("eager", "graph")}
        say(f"generated-{g}  (sequence {n}; cached vs re-run logits rel diff: eager {err['eager']:.1e}, graph "
            f"{err['graph']:.1e}; next token re-run {toks['rerun']}, eager {toks['eager']}, graph {toks['graph']})")
        for k in arms:
            extra = ""
            if k in ("eager", "graph"):
                extra = f"   rerun/this {med['rerun'] / med[k]:5.2f}x  " + \
                        ("(ranges disjoint)" if min(t["rerun"]) > max(t[k]) else "(ranges overlap)")
            say(f"  {k:6s}{med[k]:9.3f} ms [{min(t[k]):8.3f} .. {max(t[k]):8.3f}]  {wbytes / med[k] / 1e6:7.0f} GB/s{extra}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
