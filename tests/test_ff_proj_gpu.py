"""The transformer's proj_out in the tail of the fused feed-forward
(csrc/kernels/ff.hip, PROJ variant; ops.ff_fused_proj):

    z = x_in + Wp bf16(x + FF(LN3(x))) + bp     (+ the GroupNorm partials of z)

CPU: the packing round-trips, the fp32 reference built from the packed weights
equals the unfused composition, and the path is not taken on CPU or at C = 640.
GPU: the kernel against the fp32 composition, no further from it than 1.5 x
today's two launches (``ff_geglu``, then the proj_out GEMM with residual and
GroupNorm statistics) — both round to bf16 at the same points, only the fp32
summation order differs — at every segment height, its statistics against the
moments of its own output, determinism, graph replay, and the Transformer2D
with the switch on against off."""
import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import BasicTransformerBlock, Linear, Transformer2D, init_random_

C = 320


def _setup(dev, dtype, B=2, S=256, seed=0, bias=True):
    torch.manual_seed(seed)
    blk = BasicTransformerBlock(C, C // 64, 64, 1024).to(dev)
    init_random_(blk, seed=seed)
    po = Linear(C, C).to(dev)
    init_random_(po, seed=seed + 1)
    with torch.no_grad():  # non-trivial LayerNorm affine and biases
        blk.norm3.weight.uniform_(0.5, 1.5)
        blk.norm3.bias.normal_(0, 0.2)
        blk.ff.net[0].proj.bias.normal_(0, 0.3)
        blk.ff.net[2].bias.normal_(0, 0.3)
        po.bias.normal_(0, 0.3)
        if not bias:
            blk.ff.net[0].proj.bias = None
            blk.ff.net[2].bias = None
            po.bias = None
    blk, po = blk.to(dtype), po.to(dtype)
    blk.ff.prepare()
    x = (torch.randn(B, S, C, device=dev) * 2 + 0.5).to(dtype)
    xin = (torch.randn(B, S, C, device=dev) * 1.5 - 0.3).to(dtype)
    return blk, po, x, xin


def _unfused(x, xin, blk, po):
    """fp32 composition of the modules: LayerNorm -> GEGLU -> down-projection +
    residual -> proj_out + residual."""
    ff = blk.ff
    h = torch.nn.functional.layer_norm(x.float(), (C,), blk.norm3.weight.float(), blk.norm3.bias.float(),
                                       blk.norm3.eps)
    p = ff.net[0].proj
    vg = torch.nn.functional.linear(h, p.weight.float(), None if p.bias is None else p.bias.float())
    inner = vg.shape[-1] // 2
    hid = vg[..., :inner] * torch.nn.functional.gelu(vg[..., inner:])
    d = ff.net[2]
    y = x.float() + torch.nn.functional.linear(hid, d.weight.float(), None if d.bias is None else d.bias.float())
    return xin.float() + torch.nn.functional.linear(y, po.weight.float(), None if po.bias is None else po.bias.float())


def _args(blk, po, xin):
    w1p, b1p, w2p = blk.ff.fused_weights()
    return (blk.norm3.weight, blk.norm3.bias, w1p, b1p, w2p, blk.ff.net[2].bias, ops.pack_ff_proj(po.weight), po.bias,
            xin, blk.norm3.eps)


def rel_err(y, ref):
    y, ref = y.float(), ref.float()
    return ((y - ref).norm() / ref.norm()).item()


def test_pack_proj_roundtrip_cpu():
    torch.manual_seed(0)
    wp = torch.randn(C, C)
    wpp = ops.pack_ff_proj(wp)
    assert wpp.shape == (10, 10, 32, 32)
    assert torch.equal(ops.unpack_ff_proj(wpp), wp)
    # the same images as the down-projection's: a [C, I] weight through pack_ff_fused
    w2 = torch.randn(C, 1280)
    _, _, w2p = ops.pack_ff_fused(torch.randn(2560, C), None, w2)
    assert torch.equal(ops.unpack_ff_fused(torch.zeros(80, 5, 32, 64), None, w2p)[2], w2)


@pytest.mark.parametrize("bias", [True, False])
def test_ref_equals_unfused_cpu(bias):
    blk, po, x, xin = _setup("cpu", torch.float32, bias=bias)
    z = ops._ref_ff_fused_proj(x, *_args(blk, po, xin))
    ref = _unfused(x, xin, blk, po)
    assert z.shape == xin.shape
    assert torch.allclose(z, ref, atol=1e-4, rtol=1e-4), (z - ref).abs().max()
    # ops.ff_fused_proj on CPU is that reference
    assert torch.equal(ops.ff_fused_proj(x, *_args(blk, po, xin)), z)


def test_off_cpu_and_other_widths():
    """Not a HIP path on CPU; a C = 640 transformer packs nothing and keeps its proj_out GEMM."""
    blk, po, x, xin = _setup("cpu", torch.float32)
    assert ops.ff_proj_fusable(x, blk.ff.inner, x.shape[1]) == 0
    for c in (320, 640):
        t = Transformer2D(c, c // 64, 1024)
        init_random_(t, seed=3)
        xi = torch.randn(1, 8, 8, c)
        assert t._proj_tail(xi) is None
        y = t(xi, ctx=torch.randn(1, 77, 1024))
        assert y.shape == xi.shape and "_ffproj" not in t.__dict__


@pytest.fixture(scope="module")
def cases(gpu):
    """Per (B, S, bias): inputs, the fp32 CPU composition and the two-launch result, computed once."""
    from chiaswarm_amd.ops import hip_ops

    out = {}

    def get(B, S, bias):
        key = (B, S, bias)
        if key not in out:
            blk, po, x, xin = _setup(gpu, torch.bfloat16, B=B, S=S, bias=bias)
            ref = _unfused(x.cpu(), xin.cpu(), blk.cpu().float(), po.cpu().float())
            blk, po = blk.to(gpu).bfloat16(), po.to(gpu).bfloat16()
            blk.ff.prepare()
            a = _args(blk, po, xin)
            y = hip_ops.ff_geglu(x, *a[:6], a[9])
            two = ops.gemm(y, po.weight, po.bias, residual=xin, gn_rows=S)
            torch.cuda.synchronize()
            out[key] = (x, a, ref, two.cpu())
        return out[key]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [32, 64, 128])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,S", [(1, 128), (2, 256), (3, 384)])
def test_kernel_matches_fp32_and_two_launches(gpu, cases, B, S, bias, seg):
    from chiaswarm_amd.ops import hip_ops

    x, a, ref, two = cases(B, S, bias)
    z = hip_ops.ff_geglu_proj(x, *a, gn_rows=S, seg=seg)
    torch.cuda.synchronize()
    assert z.shape == a[8].shape and torch.isfinite(z.float()).all()
    err_fused, err_two = rel_err(z.cpu(), ref), rel_err(two, ref)
    print(f"ff_proj B{B} S{S} bias{int(bias)} seg{seg}: err fused {err_fused:.4e} two-launch {err_two:.4e} "
          f"ratio {err_fused / err_two:.3f}")
    assert err_fused <= 1.5 * err_two
    assert err_fused < 1.2e-2
    # GroupNorm partials: the moments of the kernel's own (rounded) output
    part, pseg = z._csk_gn
    assert pseg == seg and part.numel() == (B * S // seg) * C * 2
    zv = z.float().reshape(-1, seg, C)
    pm = part.view(-1, C, 2)
    assert torch.allclose(pm[..., 0], zv.mean(1), atol=2e-2)
    assert rel_err(pm[..., 1], zv.var(1, unbiased=False) * seg) < 2e-2
    g, b = torch.randn(C, device=gpu).bfloat16(), torch.randn(C, device=gpu).bfloat16()
    fused = hip_ops.group_norm(z, g, b, 32, 1e-5, True)
    gref = ops._ref_group_norm(z.float().cpu(), g.float().cpu(), b.float().cpu(), 32, 1e-5, True)
    assert rel_err(fused.cpu(), gref) < 1e-2


@pytest.mark.gpu
def test_kernel_rejects_partial_tiles_and_straddling_segments(gpu, cases):
    from chiaswarm_amd.ops import hip_ops

    x, a, _, _ = cases(1, 128, True)
    with pytest.raises(ValueError):  # 96 rows: no whole 128-row tile
        hip_ops.ff_geglu_proj(x[:, :96], *a[:8], a[8][:, :96], a[9], gn_rows=96, seg=32)
    with pytest.raises(ValueError):  # a 128-row segment would straddle 64-row samples
        hip_ops.ff_geglu_proj(x, *a, gn_rows=64, seg=128)


@pytest.mark.gpu
def test_kernel_deterministic_and_graph_replay(gpu, cases):
    from chiaswarm_amd.ops import hip_ops

    x, a, _, _ = cases(2, 256, True)
    run = lambda: hip_ops.ff_geglu_proj(x, *a, gn_rows=256, seg=64)  # noqa: E731
    z0, z1 = run(), run()
    assert torch.equal(z0, z1) and torch.equal(z0._csk_gn[0], z1._csk_gn[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        zc = run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(zc, z0) and torch.equal(zc._csk_gn[0], z0._csk_gn[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dup", [False, True])
def test_transformer_switch_on_vs_off(gpu, monkeypatch, dup):
    """Transformer2D at C = 320, batch 2 on a 16x16 grid (the row gates lowered):
    proj_out rides in the fused feed-forward exactly once, agrees with the
    stand-alone GEMM and hands the consumer the same statistics segments."""
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
    ctx = torch.randn(B, 77, 1024, device=gpu).bfloat16()
    kvs = [m.context_kv(ctx) for m in t.cross_modules()]
    monkeypatch.setattr(hip_ops, "FF_PROJ", True)
    n0 = hip_ops.FF_PROJ_STATS[0]
    on = t(x, kvs=kvs, dup=dup)
    assert hip_ops.FF_PROJ_STATS[0] == n0 + 1
    monkeypatch.setattr(hip_ops, "FF_PROJ", False)
    off = t(x, kvs=kvs, dup=dup)
    assert hip_ops.FF_PROJ_STATS[0] == n0 + 1
    torch.cuda.synchronize()
    assert on.shape == off.shape == (B, 16, 16, C)
    assert rel_err(on, off) < 2e-2
    assert on._csk_gn[1] == off._csk_gn[1] and on._csk_gn[0].shape == off._csk_gn[0].shape
