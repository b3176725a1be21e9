"""Depthwise NHWC conv ops on the CPU: ``ops.depthwise_conv2d`` /
``ops.depthwise_conv_transpose2d`` against an independently written float64
reference (``F.conv2d`` / ``F.conv_transpose2d(groups=C)`` on explicitly padded
input), the weight packing, the shared validation, and the K-UNet resamplers
against the formula their ``forward`` used before they called the ops."""
import pytest
import torch
import torch.nn.functional as F

from chiaswarm_amd import ops
from chiaswarm_amd.models.kunet import KDownsample2D, KUpsample2D
from tests._dwconv_ref import _abs, ref_conv64, ref_convt64


def close32(y, ref, S, k):
    """fp32 round-off: the forward bound of a k-term fp32 sum (+ bias, residual and the final rounding) is
    (k + 3) u S with u = 2^-24 and S the same expression on absolute values; doubled, because the CPU
    conv's summation order is its own."""
    assert y.shape == ref.shape and y.dtype == torch.float32
    assert bool(((y.double() - ref).abs() <= (k + 3) * 2.0 ** -23 * S).all())


CASES = [  # kh, kw, stride, padding, mode
    (3, 3, 1, 1, "zeros"), (3, 3, 2, 1, "reflect"), (4, 4, 2, 1, "reflect"), (4, 4, 1, (2, 1, 1, 2), "zeros"),
    (7, 7, 1, 3, "zeros"), (7, 7, 2, (3, 2, 1, 0), "reflect"), (1, 7, 1, (0, 3, 0, 3), "zeros"),
    (1, 7, 2, (0, 2, 0, 4), "reflect"), (3, 3, 1, (0, 2, 1, 0), "reflect"),
]


@pytest.mark.parametrize("kh,kw,stride,pad,mode", CASES)
@pytest.mark.parametrize("extras", [False, True])
def test_depthwise_conv2d_matches_fp64(kh, kw, stride, pad, mode, extras):
    torch.manual_seed(kh * 10 + kw + stride)
    B, H, W, C = 2, 9, 11, 16
    x = torch.randn(B, H, W, C)
    w = torch.randn(C, 1, kh, kw) / (kh * kw) ** 0.5
    wp = ops.pack_depthwise_weight(w)
    ho, wo = ops.conv_out_size(H, W, kh, kw, stride, pad)
    if extras:  # bias, residual, and out= as a channel slice of a wider buffer
        bias, res = torch.randn(C), torch.randn(B, ho, wo, C)
        buf = torch.full((B, ho, wo, C + 8), 7.0)
        y = ops.depthwise_conv2d(x, wp, bias, stride, pad, mode, residual=res, out=buf[..., 8:])
        assert y.data_ptr() == buf[..., 8:].data_ptr()
        assert bool((buf[..., :8] == 7.0).all())
    else:
        bias = res = None
        y = ops.depthwise_conv2d(x, wp, stride=stride, padding=pad, pad_mode=mode)
    S = ref_conv64(x.abs(), w.abs(), _abs(bias), stride, pad, mode, _abs(res))
    close32(y, ref_conv64(x, w, bias, stride, pad, mode, res), S, kh * kw)


@pytest.mark.parametrize("k,pad,mode,crop", [(4, 1, "reflect", 3), (3, 0, "zeros", 1), (4, (1, 0, 2, 1), "zeros", 0),
                                             (7, 2, "reflect", 4)])
@pytest.mark.parametrize("bias", [False, True])
def test_depthwise_conv_transpose2d_matches_fp64(k, pad, mode, crop, bias):
    torch.manual_seed(k + crop)
    B, H, W, C = 2, 5, 7, 8
    x = torch.randn(B, H, W, C)
    w = torch.randn(C, 1, k, k) / k
    b = torch.randn(C) if bias else None
    ref = ref_convt64(x, w, b, pad, mode, crop)
    buf = torch.zeros(B, ref.shape[1], ref.shape[2], C + 8)
    y = ops.depthwise_conv_transpose2d(x, ops.pack_depthwise_weight(w), b, in_padding=pad, pad_mode=mode, crop=crop,
                                       out=buf[..., :C])
    close32(y, ref, ref_convt64(x.abs(), w.abs(), _abs(b), pad, mode, crop), k * k)
    assert bool((buf[..., C:] == 0).all())


def test_pack_depthwise_weight_layouts():
    w = torch.randn(24, 1, 3, 5, dtype=torch.bfloat16)
    wp = ops.pack_depthwise_weight(w)
    assert wp.dtype == torch.float32 and wp.shape == (3, 5, 24) and wp.is_contiguous()
    assert torch.equal(wp.permute(2, 0, 1), w[:, 0].float())
    assert torch.equal(ops.pack_depthwise_weight(w[:, 0]), wp)
    with pytest.raises(ValueError):
        ops.pack_depthwise_weight(torch.randn(8, 2, 3, 3))
    with pytest.raises(ValueError):
        ops.pack_depthwise_weight(torch.randn(8, 3))


@pytest.mark.parametrize("H,W", [(8, 8), (7, 9), (1, 2), (2, 5)])
def test_kunet_resamplers_keep_their_formula(H, W):
    """Bit-identical to the permute / F.pad(reflect) / grouped conv chain the modules ran before."""
    torch.manual_seed(H * W)
    C = 32
    x = torch.randn(2, H, W, C)
    down, up = KDownsample2D(C), KUpsample2D(C)
    assert list(down.state_dict()) == [] and list(up.state_dict()) == []
    if min(H, W) >= 2:  # reflect pad 1 needs two pixels
        xn = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
        yd = F.conv2d(xn, down.kernel.to(x.dtype), stride=2, groups=C).permute(0, 2, 3, 1).contiguous()
        yu = F.conv_transpose2d(xn, up.kernel.to(x.dtype), stride=2, padding=3, groups=C).permute(0, 2, 3, 1)
        d, u = down(x), up(x)
        assert torch.equal(d, yd) and torch.equal(u, yu.contiguous())
        assert d.shape == (2, H // 2, W // 2, C) and u.shape == (2, 2 * H, 2 * W, C)  # odd sizes round down
        assert d.is_contiguous() and u.is_contiguous()
    else:
        with pytest.raises(ValueError):
            down(x)
        with pytest.raises(ValueError):
            up(x)


def test_validation_raises_on_cpu():
    x = torch.randn(1, 6, 6, 16)
    wp = ops.pack_depthwise_weight(torch.randn(16, 1, 3, 3))
    with pytest.raises(ValueError):  # C % 8
        ops.depthwise_conv2d(torch.randn(1, 6, 6, 12), ops.pack_depthwise_weight(torch.randn(12, 1, 3, 3)))
    with pytest.raises(ValueError):  # k > 7
        ops.depthwise_conv2d(torch.randn(1, 9, 9, 16), ops.pack_depthwise_weight(torch.randn(16, 1, 8, 8)))
    with pytest.raises(ValueError):  # stride
        ops.depthwise_conv2d(x, wp, stride=3)
    with pytest.raises(ValueError):  # reflect pad >= size
        ops.depthwise_conv2d(x, wp, padding=6, pad_mode="reflect")
    with pytest.raises(ValueError):
        ops.depthwise_conv_transpose2d(x, wp, in_padding=(0, 6, 0, 0), pad_mode="reflect")
    with pytest.raises(ValueError):  # weights must be the packed fp32 layout
        ops.depthwise_conv2d(x, wp.to(torch.bfloat16))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, torch.randn(16, 3, 3))
    with pytest.raises(ValueError):  # unknown pad mode, negative crop, wrong out / residual / bias shapes
        ops.depthwise_conv2d(x, wp, pad_mode="edge")
    with pytest.raises(ValueError):
        ops.depthwise_conv_transpose2d(x, wp, crop=-1)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, wp, out=torch.empty(1, 6, 6, 16))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, wp, residual=torch.empty(1, 6, 6, 16))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, wp, bias=torch.zeros(8))
    with pytest.raises(ValueError):  # kernel larger than the padded input
        ops.depthwise_conv2d(torch.randn(1, 2, 2, 16), wp)
