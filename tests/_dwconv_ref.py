"""float64 references of the depthwise conv ops for tests/test_dwconv*.py (a plain
helper module): ``F.conv2d`` / ``F.conv_transpose2d(groups=C)`` on explicitly
padded input, written independently of ``ops._ref_depthwise_*``.  Applied to
absolute values they give the magnitude sum S of the error bounds."""
import torch.nn.functional as F

from chiaswarm_amd import ops


def _pad64(x, pad, mode):
    pt, pl, pb, pr = ops.norm_padding(pad)
    xn = x.double().permute(0, 3, 1, 2)
    return F.pad(xn, (pl, pr, pt, pb), mode="reflect" if mode == "reflect" else "constant")


def _abs(t):
    return None if t is None else t.abs()


def ref_conv64(x, w, bias, stride, pad, mode, residual):
    """w: PyTorch depthwise layout [C, 1, kh, kw]."""
    y = F.conv2d(_pad64(x, pad, mode), w.double(), None if bias is None else bias.double(), stride=stride,
                 groups=x.shape[-1]).permute(0, 2, 3, 1)
    return y if residual is None else y + residual.double()


def ref_convt64(x, w, bias, pad, mode, crop):
    return F.conv_transpose2d(_pad64(x, pad, mode), w.double(), None if bias is None else bias.double(), stride=2,
                              padding=crop, groups=x.shape[-1]).permute(0, 2, 3, 1)


def unpack(wp):
    """packed [kh, kw, C] -> PyTorch depthwise [C, 1, kh, kw]"""
    return wp.permute(2, 0, 1).unsqueeze(1)


def conv_pair(x, wp, bias, stride, pad, mode, residual):
    """(ref, S) of ``ops.depthwise_conv2d`` in float64 on the CPU from the tensors as they are."""
    c = lambda t: None if t is None else t.detach().cpu().double()  # noqa: E731
    x, w, bias, residual = c(x), unpack(c(wp)), c(bias), c(residual)
    return (ref_conv64(x, w, bias, stride, pad, mode, residual).contiguous(),
            ref_conv64(x.abs(), w.abs(), _abs(bias), stride, pad, mode, _abs(residual)).contiguous())


def convt_pair(x, wp, bias, pad, mode, crop):
    """(ref, S) of ``ops.depthwise_conv_transpose2d``."""
    c = lambda t: None if t is None else t.detach().cpu().double()  # noqa: E731
    x, w, bias = c(x), unpack(c(wp)), c(bias)
    return (ref_convt64(x, w, bias, pad, mode, crop).contiguous(),
            ref_convt64(x.abs(), w.abs(), _abs(bias), pad, mode, crop).contiguous())
