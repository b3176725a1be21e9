"""The self-attention out-projection as the prologue of the fused
cross-attention sub-block (csrc/kernels/xattn.hip, PRE variant;
ops.xattn_block(pre=...)):

    x = bf16(h0 + O Wo1^T + bo1),   y = x + Attn2(LayerNorm2(x))

x is formed in registers and never stored.  CPU: the column permutation of the
folded query weight round-trips, the reference equals the unfused fp32
composition, and the path is not taken on CPU or at C = 640.  GPU: the kernel
against the fp32 composition, no further from it than 1.5 x today's chain (the
out-projection GEMM, then ``xattn_block``) — both round x to bf16, only the
fp32 summation order differs — for the full batch and for both CFG halves
from one (source row m % src_rows), its row statistics, determinism, graph
replay, and the Transformer2D with all fused tails on against off.  The
prologue variant has the 8-wave workgroup only."""
import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import BasicTransformerBlock, Transformer2D, init_random_

C = 320


def _setup(dev, dtype, B=2, S=256, Skv=77, seed=0, Bsrc=None):
    torch.manual_seed(seed)
    blk = BasicTransformerBlock(C, C // 64, 64, 1024).to(dev)
    init_random_(blk, seed=seed)
    with torch.no_grad():  # non-trivial LayerNorm affine and biases
        blk.norm2.weight.uniform_(0.5, 1.5)
        blk.norm2.bias.normal_(0, 0.2)
        blk.attn1.to_out[0].bias.normal_(0, 0.3)
        blk.attn2.to_out[0].bias.normal_(0, 0.3)
    blk = blk.to(dtype)
    bs = B if Bsrc is None else Bsrc
    o = torch.randn(bs, S, C, device=dev).to(dtype)
    h0 = (torch.randn(bs, S, C, device=dev) * 2 + 0.5).to(dtype)
    kv = blk.attn2.context_kv(torch.randn(B, Skv, 1024, device=dev).to(dtype))
    return blk, o, h0, kv


def _unfused(o, h0, blk, kv):
    """fp32 composition of the modules: out-projection + residual, LayerNorm ->
    to_q -> softmax attention over the context K/V -> to_out + residual."""
    a1, a2 = blk.attn1, blk.attn2
    x = h0.float() + o.float() @ a1.to_out[0].weight.float().t() + a1.to_out[0].bias.float()
    x = x.repeat(kv.shape[0] // x.shape[0], 1, 1)
    h = torch.nn.functional.layer_norm(x, (C,), blk.norm2.weight.float(), blk.norm2.bias.float(), blk.norm2.eps)
    q = h @ a2.to_q.weight.float().t()
    b, s, c = x.shape
    H, D = kv.shape[3], kv.shape[4]
    k, v = kv[:, :, 0].float(), kv[:, :, 1].float()
    att = torch.softmax(q.view(b, s, H, D).transpose(1, 2) @ k.permute(0, 2, 3, 1) * a2.scale, -1)
    oo = (att @ v.transpose(1, 2)).transpose(1, 2).reshape(b, s, c)
    return oo @ a2.to_out[0].weight.float().t() + a2.to_out[0].bias.float() + x, x


def _folded(blk):
    a2 = blk.attn2
    return ops.fold_layer_norm(a2.to_q.weight, a2.to_q.bias, blk.norm2.weight, blk.norm2.bias)


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_permute_roundtrip_cpu():
    torch.manual_seed(0)
    w = torch.randn(C, C)
    wp = ops.permute_xattn_q(w)
    assert torch.equal(ops.unpermute_xattn_q(wp), w)
    # position 8 g + j of a 32-block holds column 4 g + j (j < 4) or 16 + 4 g + j - 4
    assert torch.equal(wp[:, 32 + 8 * 2 + 1], w[:, 32 + 4 * 2 + 1]) and torch.equal(wp[:, 8 * 3 + 6], w[:, 16 + 12 + 2])
    # a row's sum — the LayerNorm fold's colsum — does not depend on the order (up to fp32 summation order)
    assert torch.allclose(wp.sum(1), w.sum(1), atol=1e-4)


@pytest.mark.parametrize("Bsrc", [None, 1])
def test_ref_equals_unfused_cpu(Bsrc):
    blk, o, h0, kv = _setup("cpu", torch.float32, Bsrc=Bsrc)
    a1, a2 = blk.attn1, blk.attn2
    w2, colsum, b2 = _folded(blk)
    y = ops.xattn_block(None, ops.permute_xattn_q(w2), colsum, b2, kv, a2.to_out[0].weight, a2.to_out[0].bias,
                        blk.norm2.eps, a2.scale, o.shape[1], pre=(o, h0, a1.to_out[0].weight, a1.to_out[0].bias),
                        batch=kv.shape[0])
    ref, _ = _unfused(o, h0, blk, kv)
    assert y.shape == ref.shape
    assert torch.allclose(y, ref, atol=1e-4, rtol=1e-4), (y - ref).abs().max()


def test_off_cpu_and_other_widths():
    blk, o, h0, kv = _setup("cpu", torch.float32)
    assert not ops.xattn_pre_fusable(o, kv, o.shape[1]) and not ops.xattn_pre_fusable(o, kv, o.shape[1], dup=True)
    from chiaswarm_amd.ops import hip_ops

    kv640 = torch.empty(8, 77, 2, 10, 64, dtype=torch.bfloat16)
    assert not hip_ops.xattn_pre_ok(torch.empty(8, 4096, 640, dtype=torch.bfloat16), kv640, 4096)
    kv320 = torch.empty(8, 77, 2, 5, 64, dtype=torch.bfloat16)
    assert hip_ops.xattn_pre_ok(torch.empty(8, 4096, 320, dtype=torch.bfloat16), kv320, 4096)
    assert hip_ops.xattn_pre_ok(torch.empty(4, 4096, 320, dtype=torch.bfloat16), kv320, 4096, dup=True)
    assert not hip_ops.xattn_pre_ok(torch.empty(1, 4096, 320, dtype=torch.bfloat16), kv320, 4096)  # the grid gate


@pytest.fixture(scope="module")
def cases(gpu):
    """Per (B, S, Skv, half): operands, the fp32 CPU composition (y and x), and the bf16 x and y of today's
    chain (out-projection GEMM, dup2 for the halves, xattn_block), computed once."""
    from chiaswarm_amd.ops import hip_ops

    out = {}

    def get(B, S, Skv, half):
        key = (B, S, Skv, half)
        if key not in out:
            blk, o, h0, kv = _setup(gpu, torch.bfloat16, B=B, S=S, Skv=Skv, Bsrc=B // 2 if half else None)
            ref, xref = _unfused(o.cpu(), h0.cpu(), blk.cpu().float(), kv.cpu().float())
            blk = blk.to(gpu).bfloat16()
            a1, a2 = blk.attn1, blk.attn2
            w2, colsum, b2 = _folded(blk)
            x = ops.gemm(o, a1.to_out[0].weight, a1.to_out[0].bias, residual=h0)
            if half:
                x = ops.dup2(x)
            two = hip_ops.xattn_block(x, w2, colsum, b2, kv, a2.to_out[0].weight, a2.to_out[0].bias, blk.norm2.eps,
                                      a2.scale, S)
            torch.cuda.synchronize()
            args = (ops.permute_xattn_q(w2), colsum, b2, kv, a2.to_out[0].weight, a2.to_out[0].bias, blk.norm2.eps,
                    a2.scale, S)
            pre = (o, h0, a1.to_out[0].weight, a1.to_out[0].bias)
            out[key] = (args, pre, ref, xref, x.cpu().float(), two.cpu())
        return out[key]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,Skv,half", [(1, 128, 77, False), (2, 256, 77, False), (2, 128, 1, False),
                                          (2, 256, 80, False), (2, 256, 77, True), (2, 128, 1, True),
                                          (2, 256, 80, True)])
def test_kernel_matches_fp32_and_two_launches(gpu, monkeypatch, cases, B, S, Skv, half):
    """src_rows = M everywhere, and src_rows = M / 2 (both CFG halves from one) at the even batches."""
    from chiaswarm_amd.ops import hip_ops

    monkeypatch.setattr(hip_ops, "XATTN_MIN_WG", 0)
    args, pre, ref, xref, xb, two = cases(B, S, Skv, half)
    y = hip_ops.xattn_block(None, *args, pre=pre, batch=B)
    torch.cuda.synchronize()
    assert y.shape == (B, S, C) and torch.isfinite(y.float()).all()
    yc = y.cpu()
    e_f, e_t = rel(yc, ref), rel(two, ref)
    # the residual dominates y: bound the attention branch on its own too (y minus the bf16 x the chain stores)
    d_f, d_t = rel(yc.float() - xb, ref - xref), rel(two.float() - xb, ref - xref)
    print(f"xattn_pre B{B} S{S} Skv{Skv} half{int(half)}: y err fused {e_f:.4e} two-launch {e_t:.4e} ratio "
          f"{e_f / e_t:.3f}; y - x err fused {d_f:.4e} two-launch {d_t:.4e} ratio {d_f / d_t:.3f}")
    assert e_f <= 1.5 * e_t and d_f <= 1.5 * d_t
    assert e_f < 1e-2 and d_f < 2e-2
    rp, nparts, pcols = y._csk_rows
    assert nparts == 1 and pcols == C
    st = rp.view(-1, 2).cpu()
    yf = yc.float().view(-1, C)
    assert torch.allclose(st[:, 0], yf.mean(1), atol=2e-3, rtol=1e-3)
    assert torch.allclose(st[:, 1], ((yf - yf.mean(1, keepdim=True)) ** 2).sum(1), rtol=2e-3, atol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_kernel_deterministic_and_graph_replay(gpu, cases, half):
    from chiaswarm_amd.ops import hip_ops

    args, pre = cases(2, 256, 77, half)[:2]
    run = lambda: hip_ops.xattn_block(None, *args, pre=pre, batch=2)  # noqa: E731
    y0, y1 = run(), run()
    assert torch.equal(y0, y1) and torch.equal(y0._csk_rows[0], y1._csk_rows[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yc = run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yc, y0) and torch.equal(yc._csk_rows[0], y0._csk_rows[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dup", [False, True])
def test_transformer_all_switches_on_vs_off(gpu, monkeypatch, dup):
    """Transformer2D at C = 320, batch 2 on a 16x16 grid (the row gates lowered):
    each fused tail runs exactly once — the prologue (same batch, or doubling
    it under ``dup`` from a half-batch input) and proj_out in the feed-forward —
    and the result agrees with all three switches off."""
    from chiaswarm_amd.ops import hip_ops

    monkeypatch.setattr(hip_ops, "FF_MIN_ROWS", 128)
    monkeypatch.setattr(hip_ops, "XATTN_MIN_WG", 1)
    monkeypatch.setattr(hip_ops, "XIN_MIN_ROWS", 128)
    torch.manual_seed(0)
    t = Transformer2D(C, C // 64, 1024).to(gpu)
    init_random_(t, seed=2)
    t = t.bfloat16()
    B = 2
    x = torch.randn(1 if dup else B, 16, 16, C, device=gpu).bfloat16()
    kvs = [m.context_kv(torch.randn(B, 77, 1024, device=gpu).bfloat16()) for m in t.cross_modules()]
    for name in ("XATTN_PRE", "XATTN_DUP", "FF_PROJ"):
        monkeypatch.setattr(hip_ops, name, True)
    stats = (hip_ops.XATTN_PRE_STATS, hip_ops.XATTN_DUP_STATS, hip_ops.FF_PROJ_STATS)
    n0 = [s[0] for s in stats]
    on = t(x, kvs=kvs, dup=dup)
    assert [s[0] - n for s, n in zip(stats, n0)] == ([0, 1, 1] if dup else [1, 0, 1])
    for name in ("XATTN_PRE", "XATTN_DUP", "FF_PROJ"):
        monkeypatch.setattr(hip_ops, name, False)
    off = t(x, kvs=kvs, dup=dup)
    assert [s[0] - n for s, n in zip(stats, n0)] == ([0, 1, 1] if dup else [1, 0, 1])
    torch.cuda.synchronize()
    assert on.shape == off.shape == (B, 16, 16, C)
    assert rel(on, off) < 2e-2
