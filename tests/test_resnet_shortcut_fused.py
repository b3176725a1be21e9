"""ResnetBlock2D with its 1x1 shortcut folded into conv2 as extra K segments
(``ops.SC_FUSE``, ``ops.conv2d(extra=...)``) against the unfused block.

CPU: the plain-PyTorch definitions; fused and unfused are the same math
reassociated, so they agree to fp32 round-off.  GPU: both arms against the
fp32 twin of the same bf16 weights, within the model-parity bound of
tests/test_models_gpu.py (relative L2 error <= 2e-2)."""
import copy

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import ResnetBlock2D, init_random_, prepare_model


class _ScFuse:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = ops.SC_FUSE
        ops.SC_FUSE = self.on

    def __exit__(self, *exc):
        ops.SC_FUSE = self.old


def _block(cin, cout, groups=32, seed=1, temb=24):
    blk = ResnetBlock2D(cin, cout, temb_channels=temb, groups=groups).eval().requires_grad_(False)
    init_random_(blk, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():  # init_random_ zeroes the biases: the folded bias must see two non-zero ones
        for m in (blk.conv2, blk.conv_shortcut):
            if m is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return prepare_model(blk)


def _count_extra(monkeypatch):
    """number of ops.conv2d calls that carried extra K segments"""
    n = [0]
    real = ops.conv2d

    def conv2d(*a, **kw):
        n[0] += kw.get("extra") is not None
        return real(*a, **kw)

    monkeypatch.setattr(ops, "conv2d", conv2d)
    return n


@torch.no_grad()
def test_forward_fused_matches_unfused_cpu(monkeypatch):
    n = _count_extra(monkeypatch)
    blk = _block(64, 128)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 6, 5, 64, generator=g)
    tp = torch.randn(2, 128, generator=g)
    with _ScFuse(False):
        want = blk(x, tp)
        assert n[0] == 0
    with _ScFuse(True):
        got = blk(x, tp)
        assert n[0] == 1, "the fused arm did not pass the shortcut source to conv2"
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5 * want.abs().max().item())


@torch.no_grad()
def test_forward_cat_fused_matches_unfused_cpu(monkeypatch):
    n = _count_extra(monkeypatch)
    blk = _block(192, 128)
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(2, 4, 4, 128, generator=g), torch.randn(2, 4, 4, 64, generator=g)
    tp = torch.randn(2, 128, generator=g)
    with _ScFuse(False):
        want = blk.forward_cat(a, b, tp)
        assert n[0] == 0
    with _ScFuse(True):
        got = blk.forward_cat(a, b, tp)
        assert n[0] == 1
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5 * want.abs().max().item())
    assert torch.allclose(got, blk(torch.cat([a, b], -1), tp), rtol=1e-5, atol=1e-5 * want.abs().max().item())


def test_state_dict_keys_unchanged():
    blk = _block(64, 128)
    with _ScFuse(True), torch.no_grad():
        blk(torch.randn(1, 4, 4, 64), torch.randn(1, 128))  # the pack exists
    want = set()
    for name, mod in (("norm1", 2), ("conv1", 2), ("time_emb_proj", 2), ("norm2", 2), ("conv2", 2),
                      ("conv_shortcut", 2)):
        want |= {f"{name}.weight", f"{name}.bias"}
    assert set(blk.state_dict().keys()) == want
    assert [k for k, _ in blk.named_buffers()] == []


@torch.no_grad()
def test_reprepare_after_inplace_shortcut_update():
    """The LoRA merge path: ``conv_shortcut.weight`` changes in place, then
    ``prepare_model``; the fused output follows the new weight."""
    blk = _block(64, 128)
    g = torch.Generator().manual_seed(2)
    x, tp = torch.randn(1, 4, 4, 64, generator=g), torch.randn(1, 128, generator=g)
    with _ScFuse(True):
        before = blk(x, tp)
        blk.conv_shortcut.weight.add_(torch.randn(blk.conv_shortcut.weight.shape, generator=g) * 0.05)
        prepare_model(blk)
        after = blk(x, tp)
    with _ScFuse(False):
        want = blk(x, tp)
    assert not torch.allclose(after, before, rtol=1e-3, atol=1e-3)
    assert torch.allclose(after, want, rtol=1e-5, atol=1e-5 * want.abs().max().item())


@torch.no_grad()
def test_fused_pack_replaces_conv2_packed_copy():
    blk = _block(64, 128)
    assert blk.conv2.wp is not None
    with _ScFuse(True):
        blk(torch.randn(1, 4, 4, 64), torch.randn(1, 128))
    assert blk.conv2.wp is None and blk.conv1.wp is not None
    with _ScFuse(False):  # the unfused path rebuilds its own copy on demand
        blk(torch.randn(1, 4, 4, 64), torch.randn(1, 128))
    assert blk.conv2.wp is not None


@torch.no_grad()
def test_channels_not_multiple_of_64_stay_unfused(monkeypatch):
    n = _count_extra(monkeypatch)
    blk = _block(32, 48, groups=8)
    g = torch.Generator().manual_seed(3)
    x, tp = torch.randn(2, 4, 4, 32, generator=g), torch.randn(2, 48, generator=g)
    with _ScFuse(False):
        want = blk(x, tp)
    with _ScFuse(True):
        got = blk(x, tp)
        a, b = x[..., :16].contiguous(), x[..., 16:].contiguous()
        cat = blk.forward_cat(a, b, tp)
    assert n[0] == 0
    assert torch.equal(got, want) and torch.equal(cat, want)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _rel(y, ref):
    return ((y.float().cpu() - ref).norm() / ref.norm()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("with_next_norm", [False, True])
@pytest.mark.parametrize("cat", [False, True])
@torch.no_grad()
def test_resnet_fused_gpu(gpu, monkeypatch, cat, with_next_norm):
    """forward 64 -> 128 and forward_cat (128 | 64) -> 128 at B = 2, 16x16, 32
    groups: SC_FUSE on and off against the fp32 twin; the fused arm launches no
    shortcut GEMM (``ops.gemm`` is never called) and its conv2 carries the segments."""
    from chiaswarm_amd.models.layers import GroupNorm
    from chiaswarm_amd.ops import hip_ops

    cin = 192 if cat else 64
    blk = _block(cin, 128, seed=7 + cat).to(torch.bfloat16)
    twin = copy.deepcopy(blk).float()
    blk = prepare_model(blk.to(gpu))
    nn_ = GroupNorm(32, 128, eps=1e-6)
    torch.nn.init.normal_(nn_.weight, 1.0, 0.2)
    torch.nn.init.normal_(nn_.bias, 0.0, 0.2)
    nn_ = nn_.to(torch.bfloat16)
    nn32 = copy.deepcopy(nn_).float()
    nn_ = nn_.to(gpu)
    g = torch.Generator().manual_seed(5)
    srcs = ([torch.randn(2, 16, 16, 128, generator=g), torch.randn(2, 16, 16, 64, generator=g)] if cat
            else [torch.randn(2, 16, 16, 64, generator=g)])
    srcs = [s.to(torch.bfloat16) for s in srcs]
    tp = torch.randn(2, 128, generator=g).to(torch.bfloat16)
    ref = twin(torch.cat([s.float() for s in srcs], -1), tp.float())
    ref_n = nn32(ref)

    gemms = [0]
    real_gemm = ops.gemm

    def gemm(*a, **kw):
        gemms[0] += 1
        return real_gemm(*a, **kw)

    monkeypatch.setattr(ops, "gemm", gemm)
    dev = [s.to(gpu) for s in srcs]
    for on in (True, False):
        with _ScFuse(on):
            gemms[0] = 0
            n0 = hip_ops.SC_FUSE_STATS[0]
            kw = {"next_norm": nn_} if with_next_norm else {}
            y = blk.forward_cat(dev[0], dev[1], tp.to(gpu), **kw) if cat else blk(dev[0], tp.to(gpu), **kw)
            yn = nn_(y)
            torch.cuda.synchronize()
            if on:
                assert gemms[0] == 0, "the fused arm launched a shortcut GEMM"
                assert hip_ops.SC_FUSE_STATS[0] == n0 + 1
            else:
                assert gemms[0] == (2 if cat else 1) and hip_ops.SC_FUSE_STATS[0] == n0
        e, en = _rel(y, ref), _rel(yn, ref_n)
        print(f"cat={cat} next_norm={with_next_norm} SC_FUSE={int(on)}: rel err {e:.3e}, normed {en:.3e}")
        assert e <= 2e-2 and en <= 2e-2
