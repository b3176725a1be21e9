"""Per-element error bound for the bf16 conv kernels (a plain helper module).

``conv_ref64`` evaluates the conv as ``ops._ref_conv2d`` defines it,
y = act(conv(x, w) + bias + bias2d) * out_scale + residual, in float64 on the
CPU from the bf16 tensors as they are (bf16 inputs are exact in float64, so
only the kernel's own arithmetic is measured), together with the same
expression on absolute values,

    S = (conv(|x|, |w|) + |bias| + |bias2d|) * |out_scale| + |residual|.

``assert_bf16_close`` then requires of every output element

    |y - ref| <= 2^-8 |ref| + (K + 4) 2^-22 S

* 2^-8 |ref|: the one round-to-nearest-even to bf16 at the store (half an ulp
  of an 8-bit significand is at most 2^-8 relative);
* (K + 4) 2^-22 S: the standard forward bound gamma_n * sum|terms| of an fp32
  (u = 2^-24) sum of K products plus the epilogue's few operations, times 4
  because the MFMA's internal accumulation order is not ours.

Only ``act`` None and ``"lrelu"`` are allowed: leaky ReLU is one fp32 multiply
and 1-Lipschitz, so the bound on the pre-activation value carries over.

A whole-tensor relative error cannot see one wrong element or one wrong row of
a large output; this bound does, and reports where.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

ROUND = 2.0 ** -8     # one RNE to bf16
UNIT = 2.0 ** -22     # 4 * fp32 unit roundoff
ACTS = (None, "lrelu")


def _pad4(padding):
    if isinstance(padding, int):
        return padding, padding, padding, padding
    pt, pl, pb, pr = padding
    return pt, pl, pb, pr


def _conv64(x, w, stride, padding, up2x, dilation):
    """NHWC float64 conv of x [B, H, W, Cin] with packed weights [Cout, kh, kw, Cin]."""
    xn = x.permute(0, 3, 1, 2)
    if up2x:
        xn = xn.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)  # nearest x2, exact
    pt, pl, pb, pr = _pad4(padding)
    y = F.conv2d(F.pad(xn, (pl, pr, pt, pb)), w.permute(0, 3, 1, 2), None, stride=stride, dilation=dilation)
    return y.permute(0, 2, 3, 1)


def conv_ref64(x, wp, bias=None, stride=1, padding=1, up2x=False, bias2d=None, act=None, out_scale=1.0, dilation=1,
               residual=None):
    """(ref, S): the float64 reference and its absolute-value twin, [B, Ho, Wo, Cout] on the CPU."""
    if act not in ACTS:
        raise ValueError(f"conv_ref64: the bound is derived for act in {ACTS}, not {act!r}")
    d = lambda t: None if t is None else t.detach().to("cpu", torch.float64)  # noqa: E731
    x, wp, bias, bias2d, residual = d(x), d(wp), d(bias), d(bias2d), d(residual)
    ref = _conv64(x, wp, stride, padding, up2x, dilation)
    S = _conv64(x.abs(), wp.abs(), stride, padding, up2x, dilation)
    if bias is not None:
        ref = ref + bias
        S = S + bias.abs()
    if bias2d is not None:
        ref = ref + bias2d[:, None, None, :]
        S = S + bias2d.abs()[:, None, None, :]
    if act == "lrelu":
        ref = F.leaky_relu(ref, 0.2)
    ref = ref * out_scale
    S = S * abs(out_scale)
    if residual is not None:
        ref = ref + residual
        S = S + residual.abs()
    return ref.contiguous(), S.contiguous()


def bf16_ratio(y, ref, S, K):
    """|y - ref| / tol per element (float64, CPU); <= 1 everywhere means within the bound."""
    y = y.detach().to("cpu", torch.float64)
    if y.shape != ref.shape:
        raise AssertionError(f"shape {tuple(y.shape)} != reference {tuple(ref.shape)}")
    tol = ROUND * ref.abs() + (K + 4) * UNIT * S
    err = (y - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(y), ratio, torch.full_like(ratio, float("inf")))
    return ratio, err, tol


def assert_bf16_close(y, ref, S, K, what="", tag=None):
    """Every element of ``y`` within 2^-8 |ref| + (K + 4) 2^-22 S of ``ref``.
    Returns the worst |y - ref| / tol.  ``tag``: with CSK_NUMERICS_LOG=<file>
    set, "<tag> <worst ratio>" is appended to that file (measurement runs)."""
    ratio, err, tol = bf16_ratio(y, ref, S, K)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    log = os.environ.get("CSK_NUMERICS_LOG")
    if log and tag is not None:
        with open(log, "a") as f:
            f.write(f"{tag} {worst:.4f} {what}\n")
    bad = ratio > 1.0
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()[:8].tolist()
        rows = "\n".join(
            f"  (b, oh, ow, c) = {tuple(i)}: y = {float(y[tuple(i)]):.6g}, ref = {float(ref[tuple(i)]):.6g}, "
            f"|err| = {float(err[tuple(i)]):.3g}, tol = {float(tol[tuple(i)]):.3g}" for i in idx)
        raise AssertionError(f"{what}: {nbad} of {ratio.numel()} elements outside the bf16 bound "
                             f"(worst |y - ref| / tol = {worst:.3g}); first offenders:\n{rows}")
    return worst
