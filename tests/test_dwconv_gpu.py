"""Depthwise NHWC conv kernels (csrc/kernels/dwconv.hip) on the GPU against a
float64 CPU reference under the per-element bf16 bound of tests/_numerics.py,

    |y - ref| <= 2^-8 |ref| + (K + 4) 2^-22 S,   K = kh * kw,

with ``ref`` and ``S`` computed from the bf16 inputs and the packed fp32 weights
(S: the same expression on |w|, |x|, |bias|, |residual|).  Shapes are the
smallest that can break the kernel: one channel vector, ragged and several
channel blocks, inputs smaller than the kernel, and every output size one off
the workgroup tile seams, whose dimensions come from ``hip_ops``.  Both forward
variants (LDS halo, direct) run every forward case."""
import itertools

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.ops import hip_ops
from tests._dwconv_ref import conv_pair, convt_pair
from tests._numerics import assert_bf16_close

pytestmark = pytest.mark.gpu

TH, TW, CB = hip_ops.DWCONV_TH, hip_ops.DWCONV_TW, hip_ops.DWCONV_CB
VARIANTS = hip_ops.DWCONV_VARIANTS
SEAMS = [(TH * a + dh, TW * b + dw) for a in (1, 2) for b in (1, 2) for dh in (-1, 1) for dw in (-1, 1)]


def bf(*shape, dev, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def weights(C, kh, kw, dev):
    return ops.pack_depthwise_weight(torch.randn(C, 1, kh, kw, device=dev) / (kh * kw) ** 0.5)


def check_conv(dev, B, H, W, C, kh, kw, stride, pad, mode, variant, bias=True, residual=True, what=""):
    x, wp = bf(B, H, W, C, dev=dev), weights(C, kh, kw, dev)
    b = bf(C, dev=dev) if bias else None
    ho, wo = ops.conv_out_size(H, W, kh, kw, stride, pad)
    r = bf(B, ho, wo, C, dev=dev) if residual else None
    y = hip_ops.depthwise_conv2d(x, wp, b, stride, ops.norm_padding(pad), mode, r, None, (ho, wo), variant=variant)
    assert y.shape == (B, ho, wo, C) and y.dtype == torch.bfloat16 and y.is_contiguous()
    ref, S = conv_pair(x, wp, b, stride, pad, mode, r)
    assert_bf16_close(y, ref, S, kh * kw, f"{what} {variant} {B}x{H}x{W}x{C} k{kh}x{kw} s{stride} pad {pad} {mode}")


def test_tile_constants_match_the_library(gpu):
    from chiaswarm_amd.ops import _lib

    assert [_lib.call_int("csk_dwconv_tile", i) for i in range(3)] == [TH, TW, CB]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("C", [8, 24, 40, 96, 384])
def test_channels(gpu, C, variant):
    """One vector, a non-power-of-two, a ragged second channel block, the real widths."""
    torch.manual_seed(C)
    check_conv(gpu, 3, 5, 7, C, 3, 3, 1, 1, "zeros", variant)
    check_conv(gpu, 3, 5, 7, C, 4, 4, 2, 1, "reflect", variant)
    check_conv(gpu, 3, 9, 33, C, 7, 7, 1, 3, "zeros", variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_tiny_inputs(gpu, variant):
    torch.manual_seed(1)
    C = 24
    for k in (1, 3, 7):  # 1x1 image, zero pad: only the centre tap meets data
        check_conv(gpu, 3, 1, 1, C, k, k, 1, k // 2, "zeros", variant)
    check_conv(gpu, 3, 1, 1, C, 4, 4, 2, (2, 1, 1, 2), "zeros", variant)
    for k, s in ((3, 1), (3, 2), (4, 2)):  # 2x2 with reflect pad 1 (the largest reflect pad it takes)
        check_conv(gpu, 3, 2, 2, C, k, k, s, 1, "reflect", variant)
    check_conv(gpu, 3, 3, 3, C, 7, 7, 1, 3, "zeros", variant)  # input smaller than the kernel
    check_conv(gpu, 3, 3, 3, C, 7, 7, 1, 2, "reflect", variant)  # ... one output, all of it reflections
    check_conv(gpu, 3, 3, 3, C, 7, 7, 2, (2, 2, 2, 2), "reflect", variant)


KERNELS = [(3, 3), (4, 4), (7, 7), (1, 7), (7, 1)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kh,kw", KERNELS)
def test_kernel_padding_matrix(gpu, kh, kw, variant):
    """Strides 1 and 2 over odd and even sizes, symmetric and asymmetric padding, zeros and reflect."""
    torch.manual_seed(kh * 8 + kw)
    sym = (kh // 2, kw // 2, kh // 2, kw // 2)
    asym = (min(kh - 1, 2), 0, min(kh - 1, 1), min(kw - 1, 3))
    for (H, W), stride, pad, mode in itertools.product([(5, 7), (9, 33), (6, 8)], (1, 2), (sym, asym),
                                                       ("zeros", "reflect")):
        check_conv(gpu, 3, H, W, 40, kh, kw, stride, pad, mode, variant, bias=(H != 6), residual=(H != 5))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kh,kw,stride,mode", [(3, 3, 1, "zeros"), (7, 7, 1, "reflect"), (7, 7, 1, "zeros"),
                                               (4, 4, 2, "reflect"), (3, 3, 2, "zeros")])
def test_tile_seams(gpu, kh, kw, stride, mode, variant):
    """Every output size (TH a +- 1, TW b +- 1), a, b in {1, 2}; at stride 2 from the even and the odd input
    size that give it."""
    torch.manual_seed(kh + stride)
    p = kh // 2 if kh % 2 else 1
    for ho, wo in SEAMS:
        for odd in ((0,) if stride == 1 else (0, 1)):
            H = (ho - 1) * stride + kh - 2 * p + odd
            W = (wo - 1) * stride + kw - 2 * p + odd
            assert ops.conv_out_size(H, W, kh, kw, stride, p) == (ho, wo)
            check_conv(gpu, 1 + odd, H, W, 72, kh, kw, stride, p, mode, variant, what=f"seam {ho}x{wo}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kh,kw,stride,pad,mode", [(7, 7, 1, 3, "zeros"), (4, 4, 2, 1, "reflect"),
                                                   (3, 3, 1, (1, 0, 2, 1), "reflect")])
def test_channel_slice_views(gpu, kh, kw, stride, pad, mode, variant):
    """x, residual and out are channel slices of wider buffers; nothing outside the output slice changes."""
    torch.manual_seed(kh)
    B, H, W, C = 3, TH + 1, TW + 3, 40
    ho, wo = ops.conv_out_size(H, W, kh, kw, stride, pad)
    xbuf, rbuf, obuf = bf(B, H, W, C + 24, dev=gpu), bf(B, ho, wo, C + 8, dev=gpu), bf(B, ho, wo, C + 48, dev=gpu)
    x, r, out = xbuf[..., 16:16 + C], rbuf[..., 8:], obuf[..., 8:8 + C]
    wp, b = weights(C, kh, kw, gpu), torch.randn(C, device=gpu)  # an fp32 bias
    keep, xkeep = obuf.clone(), xbuf.clone()
    before = hip_ops.DWCONV_STATS[0]
    y = hip_ops.depthwise_conv2d(x, wp, b, stride, ops.norm_padding(pad), mode, r, out, (ho, wo), variant=variant)
    assert hip_ops.DWCONV_STATS[0] == before + 1
    assert y.data_ptr() == out.data_ptr()
    ref, S = conv_pair(x, wp, b, stride, pad, mode, r)
    assert_bf16_close(y, ref, S, kh * kw, f"views {variant}")
    assert torch.equal(obuf[..., :8], keep[..., :8]) and torch.equal(obuf[..., 8 + C:], keep[..., 8 + C:])
    assert torch.equal(xbuf, xkeep)


def test_default_variant_and_counter(gpu):
    """``ops.depthwise_conv2d`` reaches the kernel once per call; in-place residual (out aliases it) is allowed."""
    torch.manual_seed(2)
    x, wp = bf(3, 9, 33, 96, dev=gpu), weights(96, 7, 7, gpu)
    before = hip_ops.DWCONV_STATS[0]
    y = ops.depthwise_conv2d(x, wp, None, 1, 3)
    assert hip_ops.DWCONV_STATS[0] == before + 1
    ref, S = conv_pair(x, wp, None, 1, 3, "zeros", None)
    assert_bf16_close(y, ref, S, 49, "default variant")
    for v in VARIANTS:
        assert torch.equal(hip_ops.depthwise_conv2d(x, wp, None, 1, (3,) * 4, "zeros", None, None, (9, 33), variant=v), y)
    with ops.ops_mode("reference"):
        ops.depthwise_conv2d(x, wp, None, 1, 3)
    assert hip_ops.DWCONV_STATS[0] == before + 3


TRANSPOSED = [(4, 1, "reflect", 3), (3, 0, "zeros", 1), (4, (1, 0, 2, 1), "zeros", 2), (7, 1, "reflect", 0)]


@pytest.mark.parametrize("k,pad,mode,crop", TRANSPOSED)
def test_transposed(gpu, k, pad, mode, crop):
    """The KUpsample2D geometry (reflect 1, 4x4, crop 3), a zero-padded 3x3 crop 1, and two more; sizes from one
    pixel to outputs across the tile seams."""
    torch.manual_seed(k + crop)
    for H, W in [(1, 1), (2, 3), (5, 7), (TH // 2, TW // 2 + 1), (TH + 1, TW)]:
        for C, bias in ((24, False), (72, True)):
            x, wp = bf(3, H, W, C, dev=gpu), weights(C, k, k, gpu)
            b = bf(C, dev=gpu) if bias else None
            if mode == "reflect" and min(H, W) < 2:
                with pytest.raises(ValueError):
                    ops.depthwise_conv_transpose2d(x, wp, b, pad, mode, crop)
                continue
            before = hip_ops.DWCONV_STATS[0]
            ref, S = convt_pair(x, wp, b, pad, mode, crop)
            if ref.shape[1] < 1 or ref.shape[2] < 1:
                continue
            obuf = bf(3, ref.shape[1], ref.shape[2], C + 16, dev=gpu)
            keep = obuf.clone()
            y = ops.depthwise_conv_transpose2d(x, wp, b, pad, mode, crop, out=obuf[..., 8:8 + C])
            assert hip_ops.DWCONV_STATS[0] == before + 1
            assert_bf16_close(y, ref, S, k * k, f"transposed {H}x{W}x{C} k{k} pad {pad} {mode} crop {crop}")
            assert torch.equal(obuf[..., :8], keep[..., :8]) and torch.equal(obuf[..., 8 + C:], keep[..., 8 + C:])


def test_hip_path_validation(gpu):
    x, wp = bf(1, 6, 6, 16, dev=gpu), weights(16, 3, 3, gpu)
    with pytest.raises(ValueError):  # fp32 activations
        ops.depthwise_conv2d(x.float(), wp)
    with pytest.raises(ValueError):  # a slice that starts off a 16-byte boundary
        ops.depthwise_conv2d(bf(1, 6, 6, 24, dev=gpu)[..., 4:20], wp)
    with pytest.raises(ValueError):  # channels not the contiguous dim
        ops.depthwise_conv2d(bf(1, 16, 6, 6, dev=gpu).permute(0, 2, 3, 1), wp)
    with pytest.raises(ValueError):  # weights on the host
        ops.depthwise_conv2d(x, wp.cpu())
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, wp, out=torch.empty(1, 4, 4, 16, device=gpu))
    with pytest.raises(ValueError):
        ops.depthwise_conv_transpose2d(x, wp, out=torch.empty(1, 13, 13, 16, device=gpu, dtype=torch.float32))


# ---------------------------------------------------------------------------
def _resamplers(dev):
    from chiaswarm_amd.models.kunet import KDownsample2D, KUpsample2D

    return KDownsample2D(32).to(dev).to(torch.bfloat16), KUpsample2D(32).to(dev).to(torch.bfloat16)


def test_kunet_resamplers(gpu):
    torch.manual_seed(3)
    down, up = _resamplers(gpu)
    for H, W in [(8, 8), (TH * 2 + 1, TW + 1)]:
        x = bf(3, H, W, 32, dev=gpu)
        before = hip_ops.DWCONV_STATS[0]
        d, u = down(x), up(x)
        assert hip_ops.DWCONV_STATS[0] == before + 2  # the HIP kernel ran, once each
        assert d.shape == (3, H // 2, W // 2, 32) and u.shape == (3, 2 * H, 2 * W, 32)
        assert down.wp.dtype == torch.float32 and down.wp.device == x.device
        ref, S = conv_pair(x, down.wp, None, 2, 1, "reflect", None)
        assert_bf16_close(d, ref, S, 16, f"KDownsample2D {H}x{W}")
        ref, S = convt_pair(x, up.wp, None, 1, "reflect", 3)
        assert_bf16_close(u, ref, S, 16, f"KUpsample2D {H}x{W}")


def test_graph_capture(gpu):
    """A down + up pair captured with torch.cuda.graph: replays equal eager bitwise, also on refreshed input."""
    torch.manual_seed(4)
    down, up = _resamplers(gpu)
    x = bf(2, 12, 20, 32, dev=gpu)

    def step(t):
        return up(down(t)), down(up(t))

    e0 = [t.clone() for t in step(x)]  # eager; also packs the filters outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(x)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        outs = step(x)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, e0))
    x2 = bf(2, 12, 20, 32, dev=gpu)
    x.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs]
    e1 = step(x2)
    assert all(torch.equal(a, b) for a, b in zip(got, e1))
    assert not torch.equal(got[0], e0[0])


def test_convnext_backbone(gpu):
    """A tiny ConvNeXt on the native NHWC path against the same weights in fp32 on the CPU; the yardstick is
    the torch-bf16 path (``reference`` mode) measured the same way: e_new <= 1.25 e_par per feature map."""
    from chiaswarm_amd.controlnet.annotators import ConvNextBackbone

    torch.manual_seed(5)
    dims, depths = (16, 32, 64, 128), (1, 1, 2, 1)
    m = ConvNextBackbone(dims, depths).eval().requires_grad_(False)
    with torch.no_grad():
        for st in m.encoder.stages:
            for blk in st.layers:  # at the 1e-6 init every block is an identity
                blk.layer_scale_parameter.copy_(torch.randn_like(blk.layer_scale_parameter))
    x = torch.randn(1, 3, 64, 96)
    with torch.no_grad():
        want = [f.float() for f in m(x)]
        mg = ConvNextBackbone(dims, depths).eval().requires_grad_(False)
        mg.load_state_dict(m.state_dict())
        mg = mg.to(gpu).to(torch.bfloat16)
        xg = x.to(gpu).to(torch.bfloat16)
        before = hip_ops.DWCONV_STATS[0]
        new = [f.float().cpu() for f in mg(xg)]
        assert hip_ops.DWCONV_STATS[0] == before + sum(depths)
        with ops.ops_mode("reference"):
            par = [f.float().cpu() for f in mg(xg)]
        assert hip_ops.DWCONV_STATS[0] == before + sum(depths)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    for i, (w, n, p) in enumerate(zip(want, new, par)):
        assert n.shape == w.shape
        e_new, e_par = rel(n, w), rel(p, w)
        print(f"convnext stage{i + 1}: e_new = {e_new:.5f}  e_par = {e_par:.5f}")
        assert e_new <= 1.25 * e_par, f"stage{i + 1}: e_new {e_new:.5f} > 1.25 * e_par {e_par:.5f}"
