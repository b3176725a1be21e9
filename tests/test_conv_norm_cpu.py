"""``ops.conv2d(..., norm=...)`` on the CPU / reference path: exactly the conv
followed by ``ops.group_norm`` (the HIP path may apply the norm inside a
split-K conv's reduce kernel; its definition is this composition)."""
import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.models.layers import Conv2d, GroupNorm, ResnetBlock2D, init_random_


def _inputs(dtype, B=2, H=6, W=5, Cin=8, Cout=16):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, Cin, generator=g).to(dtype)
    wp = ops.pack_conv_weight((torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(dtype))
    bias = torch.randn(Cout, generator=g).to(dtype)
    b2 = torch.randn(B, 3 * Cout, generator=g).to(dtype)[:, Cout:2 * Cout]  # a strided column slice
    res = torch.randn(B, H, W, 2 * Cout, generator=g).to(dtype)[..., :Cout]  # a channel-slice view
    gamma = (torch.randn(Cout, generator=g) + 1.0).to(dtype)
    beta = torch.randn(Cout, generator=g).to(dtype)
    return x, wp, bias, b2, res, gamma, beta


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("keep_raw", [False, True])
@pytest.mark.parametrize("extras", [False, True])
def test_conv_norm_is_conv_then_group_norm(dtype, silu, keep_raw, extras):
    x, wp, bias, b2, res, gamma, beta = _inputs(dtype)
    kw = dict(bias=bias, bias2d=b2, residual=res, out_scale=0.5) if extras else {}
    raw = ops.conv2d(x, wp, **kw)
    want = ops.group_norm(raw, gamma, beta, 4, 1e-5, silu=silu)
    got = ops.conv2d(x, wp, norm=(gamma, beta, 4, 1e-5, silu, keep_raw), **kw)
    if keep_raw:
        got, got_raw = got
        assert torch.equal(got_raw, raw)
    assert torch.is_tensor(got) and got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(got, want)


def test_conv_norm_per_sample_affine():
    x, wp, bias, _, _, gamma, beta = _inputs(torch.float32)
    g2, b2 = torch.stack([gamma, gamma * 0.5]), torch.stack([beta, beta + 1.0])
    want = ops.group_norm(ops.conv2d(x, wp, bias), g2, b2, 4, 1e-5, silu=True)
    assert torch.equal(ops.conv2d(x, wp, bias, norm=(g2, b2, 4, 1e-5, True, False)), want)


def test_conv_norm_rejects_unsupported_epilogues():
    x, wp, _, _, res, gamma, beta = _inputs(torch.float32)
    with pytest.raises(ValueError):
        ops.conv2d(x, wp, residual=res, res_scale=0.2, norm=(gamma, beta, 4, 1e-5, False, False))
    buf = torch.empty(2, 6, 5, 16)
    with pytest.raises(ValueError):  # out= is the raw output's buffer
        ops.conv2d(x, wp, out=buf, norm=(gamma, beta, 4, 1e-5, False, False))
    yn, raw = ops.conv2d(x, wp, out=buf, norm=(gamma, beta, 4, 1e-5, False, True))
    assert raw is buf and torch.equal(yn, ops.group_norm(ops.conv2d(x, wp), gamma, beta, 4, 1e-5))
    none, raw = ops.conv2d(x, wp, norm=(gamma, beta, 4, 1e-5, False, True), norm_optional=True)
    assert none is None and torch.equal(raw, ops.conv2d(x, wp))


def test_conv2d_module_norm_argument():
    torch.manual_seed(0)
    conv, norm = Conv2d(8, 16, 3, padding=1), GroupNorm(4, 16)
    with torch.no_grad():
        norm.weight.normal_(1.0, 0.3)
        norm.bias.normal_(0.0, 0.3)
        x = torch.randn(2, 5, 5, 8)
        want = norm(conv(x), silu=True)
        assert torch.equal(conv(x, norm=norm.after_conv(silu=True)), want)
        yn, raw = conv(x, norm=norm.after_conv(silu=True, keep_raw=True))
        assert torch.equal(yn, want) and torch.equal(raw, conv(x))
        c1 = Conv2d(8, 16, 1, padding=0)  # the 1x1 GEMM shortcut path
        assert torch.allclose(c1(x, norm=norm.after_conv()), norm(c1(x)), atol=1e-5, rtol=1e-5)


def test_resnet_block_unchanged_by_the_norm_argument():
    """ResnetBlock2D hands norm2 to conv1: same result as the explicit chain."""
    blk = ResnetBlock2D(8, 16, temb_channels=12, groups=4).eval()
    init_random_(blk, seed=2)
    with torch.no_grad():
        x, tp = torch.randn(2, 4, 4, 8), torch.randn(2, 16)
        h = blk.norm1(x, silu=True)
        h = blk.norm2(blk.conv1(h, bias2d=tp), silu=True)
        want = blk.conv2(h, residual=blk.conv_shortcut(x))
        assert torch.equal(blk(x, tp), want)
        a, b = x[..., :3].contiguous(), x[..., 3:].contiguous()
        assert torch.equal(blk.forward_cat(a, b, tp), want)
