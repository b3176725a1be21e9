"""The NHWC implicit-GEMM conv (gemm.hip, gemm_glds.hip, gemm8p.hip) by tile
number over a geometry x Cin x split-K matrix and over the operand layouts
``conv2d`` accepts, each output element against the float64 reference within
the bf16 bound of tests/_numerics.py.

The input gather is written once per kernel family and staging path (FAST:
Cin % 64 == 0, guarded otherwise), and the epilogue picks among four store
paths by N % 8, the pixel strides and the pointer alignment: every (tile,
geometry) case below runs Cin = 64 / 128 (FAST, one / two K-steps per tap),
96 (guarded, a tap boundary inside a K-step) and 8 (guarded, several taps per
K-step), unsplit and split-K.  Tiles 31 / 33 take their documented fallback
(tiles 11 / 26) at Cin = 96 and 8.

Bugs these cases caught:
  * g6 (1x1) at Cin = 64 / 8, g7 / g9 / g10 at Cin = 8, split = 3, every tile:
    K <= 64 leaves one effective split, the kernels still wrote fp32 partials
    to the workspace and no reduce ran, so the output was never written
    (gemm.hip dispatch now drops the workspace when the split collapses).
"""
import functools

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.ops import hip_ops
from tests._numerics import assert_bf16_close, conv_ref64

pytestmark = pytest.mark.gpu

B = 2
ACT, SCALE = "lrelu", 0.5
CINS = (64, 128, 96, 8)
SPLITS = (1, 3)
# one or more per kernel, wave layout and epilogue kind
TILES = (1, 4, 5, 11, 12, 14, 16, 25, 26, 36, 31, 33)
KERNEL_FILE = {1: "gemm", 4: "gemm", 5: "gemm", 31: "gemm8p", 33: "gemm8p"}  # others: gemm_glds

# name: (kh, kw, stride, padding (t, l, b, r), dilation, up2x, H, W)
GEOMS = {
    "g0": (3, 3, 1, (1, 1, 1, 1), 1, False, 9, 7),
    "g1": (3, 3, 2, (1, 1, 1, 1), 1, False, 17, 15),
    "g2": (3, 3, 2, (0, 0, 1, 1), 1, False, 16, 14),
    "g3": (3, 3, 1, (1, 1, 1, 1), 1, True, 5, 7),
    "g4": (3, 3, 1, (2, 2, 2, 2), 2, False, 9, 7),
    "g5": (3, 3, 1, (3, 3, 3, 3), 3, False, 5, 6),  # top and bottom taps both outside for one pixel
    "g6": (1, 1, 1, (0, 0, 0, 0), 1, False, 9, 7),
    "g7": (2, 2, 2, (0, 0, 0, 0), 1, False, 10, 14),
    "g8": (4, 4, 4, (0, 0, 0, 0), 1, False, 12, 20),
    "g9": (1, 7, 1, (0, 3, 0, 3), 1, False, 1, 61),  # the conv1d view
    "g10": (1, 3, 1, (0, 5, 0, 5), 5, False, 1, 61),
    "g11": (5, 3, 1, (2, 1, 2, 1), 1, False, 9, 7),
}
# Cout = 48: a ragged N edge on every tile; 176: two column tiles, the second ragged, at 160 wide
CASES = [(g, 48) for g in GEOMS] + [("g0", 176), ("g1", 176)]

# (tile, geometry, Cin, split) the library documents as unsupported and must refuse
# with an error: none.  Every tile takes every conv geometry; tiles 31 / 33 fall
# back for Cin % 64 != 0, and a split larger than the K-steps runs with fewer splits.
REFUSED = {}


@functools.lru_cache(maxsize=None)
def _case(geom, cin, cout):
    """bf16 operands (CPU, seeded) and their float64 reference, computed once and shared."""
    kh, kw, stride, pad, dil, up, H, W = GEOMS[geom]
    g = torch.Generator().manual_seed(1000 * int(geom[1:]) + cin + cout)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)  # noqa: E731
    Ho, Wo = ops.conv_out_size(H, W, kh, kw, stride, pad, up, dil)
    c = dict(x=r(B, H, W, cin), wp=r(cout, kh, kw, cin, scale=(kh * kw * cin) ** -0.5), bias=r(cout),
             bias2d=r(B, cout), residual=r(B, Ho, Wo, cout))  # the residual differs between the two samples
    ref, S = conv_ref64(c["x"], c["wp"], c["bias"], stride, pad, up, c["bias2d"], ACT, SCALE, dil, c["residual"])
    c.update(ref=ref, S=S, K=kh * kw * cin, oshape=(B, Ho, Wo, cout), geom=GEOMS[geom])
    return c


def _conv_ex(tile, split, x, wp, bias, bias2d, residual, out, geom):
    """csk_conv2d_ex with an explicit tile and split on the views it is given
    (xs, ys, rs, b2s are the views' strides).  Checks on the host what
    hip_ops.conv2d guarantees the kernels before it launches."""
    from chiaswarm_amd.ops import _lib
    from chiaswarm_amd.ops.hip_ops import _p, _pix_stride, _s

    kh, kw, stride, (pt, pl, pb, pr), dil, up, H, W = geom
    Bx, Hx, Wx, Cin = x.shape
    Cout = wp.shape[0]
    Ho, Wo = ops.conv_out_size(H, W, kh, kw, stride, (pt, pl, pb, pr), up, dil)
    xs, ys, rs = _pix_stride(x), _pix_stride(out), _pix_stride(residual)
    assert (Hx, Wx) == (H, W) and wp.shape == (Cout, kh, kw, Cin) and wp.is_contiguous()
    assert xs is not None and xs % 8 == 0 and Cin % 8 == 0 and x.data_ptr() % 16 == 0 and wp.data_ptr() % 16 == 0
    assert out.shape == (Bx, Ho, Wo, Cout) and residual.shape == out.shape and ys is not None and rs is not None
    assert bias.shape == (Cout,) and bias2d.shape == (Bx, Cout) and bias2d.stride(1) == 1
    for t in (x, wp, bias, bias2d, residual, out):
        assert t.dtype == torch.bfloat16 and t.is_cuda
    M = Bx * Ho * Wo
    ws = torch.empty(split * M * Cout, dtype=torch.float32, device=x.device) if split > 1 else None
    _lib.call("csk_conv2d_ex", _p(out), _p(x), _p(wp), _p(bias), _p(bias2d), bias2d.stride(0), _p(residual),
              Bx, H, W, Cin, Cout, kh, kw, stride, pt, pl, Ho, Wo, int(up), xs, ys, rs, hip_ops.ACT[ACT], SCALE, dil,
              None, tile, split, _p(ws), _s())


def _tag(tile, cin):
    if tile is None:
        return "tuned"
    if tile in (31, 33) and cin % 64:
        return "gemm_glds"  # the documented fallback
    return KERNEL_FILE.get(tile, "gemm_glds")


@pytest.mark.parametrize("geom,cout", CASES, ids=[f"{g}-N{n}" for g, n in CASES])
@pytest.mark.parametrize("tile", TILES)
def test_conv_geometry_by_tile(gpu, tile, geom, cout):
    for cin in CINS:
        c = _case(geom, cin, cout)
        d = {k: c[k].to(gpu) for k in ("x", "wp", "bias", "bias2d", "residual")}
        for split in SPLITS:
            what = f"tile {tile} {geom} Cin={cin} Cout={cout} split={split}"
            out = torch.full(c["oshape"], float("nan"), dtype=torch.bfloat16, device=gpu)  # unwritten stays NaN
            if (tile, geom, cin, split) in REFUSED:
                with pytest.raises(RuntimeError, match="hipError"):
                    _conv_ex(tile, split, d["x"], d["wp"], d["bias"], d["bias2d"], d["residual"], out, c["geom"])
                continue
            _conv_ex(tile, split, d["x"], d["wp"], d["bias"], d["bias2d"], d["residual"], out, c["geom"])
            assert_bf16_close(out, c["ref"], c["S"], c["K"], what, tag=_tag(tile, cin))


# ---------------------------------------------------------------------------
# operand layouts
# ---------------------------------------------------------------------------
def _sentinel(shape, dev):
    """A bf16 pattern (small integers, exact) that no conv output reproduces by chance."""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, device=dev) * 37) % 199 - 99).to(torch.bfloat16).reshape(shape)


def _in_slice(t, dev, width, lo):
    """``t`` (CPU) as the channel slice [lo, lo + C) of a fresh ``width``-wide device buffer."""
    buf = _sentinel(t.shape[:-1] + (width,), dev)
    view = buf[..., lo:lo + t.shape[-1]]
    view.copy_(t.to(dev))
    return view


# layout: (Cout, x (width - Cin, lo), out (width - Cout, lo), residual (width - Cout, lo) or "out", bias2d slice?)
LAYOUTS = {
    # channel slices at 16-byte offsets with three different pixel strides, bias2d a column slice
    "slices": (48, (24, 8), (16, 8), (24, 16), True),
    # out at channel 4 of a buffer with ys % 8 == 4: base only 8-byte aligned
    "out8": (48, (0, 0), (12, 4), (0, 0), False),
    # the scalar tail alone / 16-byte vectors (columns 0-15) followed by a scalar tail
    "ragged4": (4, (0, 0), (4, 0), (0, 0), False),
    "ragged20": (20, (0, 0), (4, 0), (0, 0), False),
    # out aliases residual (the ResNet / RRDB call sites)
    "inplace": (48, (0, 0), (16, 8), "out", False),
}


def _layout_case(gpu, geom, cin, layout):
    cout, (xw, xlo), (ow, olo), rl, b2slice = LAYOUTS[layout]
    c = _case(geom, cin, cout)
    x = _in_slice(c["x"], gpu, cin + xw, xlo)
    obuf = _sentinel(c["oshape"][:-1] + (cout + ow,), gpu)
    out = obuf[..., olo:olo + cout]
    if rl == "out":
        out.copy_(c["residual"].to(gpu))
        res = out
    else:
        res = _in_slice(c["residual"], gpu, cout + rl[0], rl[1])
    if b2slice:
        b2 = torch.zeros(B, 3 * cout + 8, dtype=torch.bfloat16, device=gpu)[:, cout:2 * cout]
        b2.copy_(c["bias2d"].to(gpu))
    else:
        b2 = c["bias2d"].to(gpu)
    pattern = _sentinel(obuf.shape, gpu)
    return c, x, c["wp"].to(gpu), c["bias"].to(gpu), b2, res, obuf, out, pattern, (olo, olo + cout)


def _check_layout(c, obuf, out, pattern, span, what, tag):
    lo, hi = span
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    assert torch.equal(bits(obuf[..., :lo]), bits(pattern[..., :lo])), f"{what}: channels below the slice changed"
    assert torch.equal(bits(obuf[..., hi:]), bits(pattern[..., hi:])), f"{what}: channels above the slice changed"
    assert_bf16_close(out, c["ref"], c["S"], c["K"], what, tag=tag)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cin", [64, 96])
@pytest.mark.parametrize("geom", ["g0", "g1"])
@pytest.mark.parametrize("tile", [4, 11, 26, 31, None])
def test_conv_layouts(gpu, tile, geom, cin, layout):
    for split in (SPLITS if tile is not None else (None,)):
        c, x, wp, bias, b2, res, obuf, out, pattern, span = _layout_case(gpu, geom, cin, layout)
        what = f"tile {tile} {geom} Cin={cin} {layout} split={split}"
        if tile is None:  # the tuner's own choice through the public entry
            kh, kw, stride, pad, dil, up, H, W = c["geom"]
            y = ops.conv2d(x, wp, bias, stride, pad, residual=res, up2x=up, bias2d=b2, act=ACT, out_scale=SCALE, out=out,
                           dilation=dil)
            assert y.data_ptr() == out.data_ptr()
        else:
            _conv_ex(tile, split, x, wp, bias, b2, res, out, c["geom"])
        _check_layout(c, obuf, out, pattern, span, what, _tag(tile, cin))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cin", [64, 96])
@pytest.mark.parametrize("geom", ["g0", "g1"])
def test_conv_public_entry_misaligned_x(gpu, geom, cin, layout):
    """x a slice starting at channel 4 (8-byte aligned only): the host must copy it."""
    c, _, wp, bias, b2, res, obuf, out, pattern, span = _layout_case(gpu, geom, cin, layout)
    x = _in_slice(c["x"], gpu, cin + 8, 4)
    assert x.data_ptr() % 16 == 8
    kh, kw, stride, pad, dil, up, H, W = c["geom"]
    ops.conv2d(x, wp, bias, stride, pad, residual=res, up2x=up, bias2d=b2, act=ACT, out_scale=SCALE, out=out,
               dilation=dil)
    _check_layout(c, obuf, out, pattern, span, f"tuned {geom} Cin={cin} {layout} x at channel 4", "tuned")
