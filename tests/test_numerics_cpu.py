"""The per-element bf16 bound of tests/_numerics.py, checked without a GPU: a
torch fp32-accumulate conv followed by the fp32 epilogue and one bf16 cast
stands in for the kernel.  The bound must accept it clean and reject it with
each of five localized faults."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chiaswarm_amd import ops
from tests._numerics import assert_bf16_close, bf16_ratio, conv_ref64

# kh, kw, stride, padding (t, l, b, r), dilation
GEOMS = {
    "3x3": (3, 3, 1, (1, 1, 1, 1), 1),
    "3x3s2": (3, 3, 2, (1, 1, 1, 1), 1),
    "3x3d3": (3, 3, 1, (3, 3, 3, 3), 3),
    "1x1": (1, 1, 1, (0, 0, 0, 0), 1),
}
CINS = (8, 64, 640)
B, H, W, COUT = 2, 9, 7, 16
ACT, SCALE = "lrelu", 0.5
FAULTS = ("element", "tap_last_row", "pad_shift", "res_before_scale", "bias2d_sample")


def _case(geom, cin, seed=0):
    kh, kw, stride, pad, dil = GEOMS[geom]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)  # noqa: E731
    x, wp = r(B, H, W, cin), r(COUT, kh, kw, cin, scale=(kh * kw * cin) ** -0.5)
    Ho, Wo = ops.conv_out_size(H, W, kh, kw, stride, pad, False, dil)
    return dict(x=x, wp=wp, bias=r(COUT), bias2d=r(B, COUT), residual=r(B, Ho, Wo, COUT), stride=stride, padding=pad,
                dilation=dil, K=kh * kw * cin)


def _standin(c, fault=None):
    """fp32 conv + fp32 epilogue + one bf16 cast, optionally with one fault."""
    x, wp = c["x"].float().permute(0, 3, 1, 2), c["wp"].float()
    pt, pl, pb, pr = c["padding"]
    if fault == "pad_shift":  # the gather reads one column to the left
        pl, pr = pl + 1, pr - 1

    def conv(w):
        return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w.permute(0, 3, 1, 2), None, stride=c["stride"],
                        dilation=c["dilation"]).permute(0, 2, 3, 1)

    y = conv(wp)
    if fault == "tap_last_row":  # the last output row loses the tap (0, kw // 2)
        w2 = wp.clone()
        w2[:, 0, wp.shape[2] // 2, :] = 0
        y[:, -1] = conv(w2)[:, -1]
    b2 = c["bias2d"].float()
    if fault == "bias2d_sample":
        b2 = b2[[0, 0]]
    y = F.leaky_relu(y + c["bias"].float() + b2[:, None, None, :], 0.2)
    res = c["residual"].float()
    y = (y + res) * SCALE if fault == "res_before_scale" else y * SCALE + res
    return y.to(torch.bfloat16)


def _ref(c):
    return conv_ref64(c["x"], c["wp"], c["bias"], c["stride"], c["padding"], False, c["bias2d"], ACT, SCALE,
                      c["dilation"], c["residual"])


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_bound_accepts_clean_fp32_accumulation(geom, cin):
    c = _case(geom, cin)
    ref, S = _ref(c)
    # the float64 reference is the operation ops._ref_conv2d defines
    ref32 = ops._ref_conv2d(c["x"].float(), c["wp"].float(), c["bias"].float(), c["stride"], c["padding"],
                            c["residual"].float(), False, c["bias2d"].float(), ACT, SCALE, c["dilation"])
    assert torch.allclose(ref.float(), ref32, rtol=1e-4, atol=1e-4)
    assert (S >= ref.abs() * (1 - 1e-12)).all()
    worst = assert_bf16_close(_standin(c), ref, S, c["K"], what=f"{geom} Cin={cin}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_bound_rejects_injected_fault(geom, cin, fault):
    c = _case(geom, cin)
    ref, S = _ref(c)
    y = _standin(c, None if fault == "element" else fault)
    if fault == "element":
        # one element 5 % off.  A 5 % error is an absolute one of 0.05 |ref|, and the
        # accumulation term grows with K * S, so the element with the largest |ref| / S
        # is the one where 5 % must show at every K used here
        i = tuple(int(v) for v in np.unravel_index(int((ref.abs() / S).argmax()), ref.shape))
        y = y.clone()
        y[i] = (ref[i] * 1.05).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside the bf16 bound") as e:
        assert_bf16_close(y, ref, S, c["K"], what=f"{geom} Cin={cin} {fault}")
    ratio, _, _ = bf16_ratio(y, ref, S, c["K"])
    bad = (ratio > 1.0).nonzero()
    if fault == "element":
        assert bad.tolist() == [list(i)]
    elif fault == "tap_last_row":  # a border bug reads as a border bug
        assert set(bad[:, 1].tolist()) == {ref.shape[1] - 1}
    elif fault == "bias2d_sample":
        assert set(bad[:, 0].tolist()) == {1}
    assert "(b, oh, ow, c)" in str(e.value)


def test_zeroed_pixel_fails_in_every_channel():
    c = _case("3x3", 64)
    ref, S = _ref(c)
    y = _standin(c)
    y[1, 4, 3, :] = 0
    ratio, _, _ = bf16_ratio(y, ref, S, c["K"])
    assert (ratio[1, 4, 3] > 1.0).all() and int((ratio > 1.0).sum()) == COUT


def test_nan_and_shape_are_rejected():
    c = _case("1x1", 8)
    ref, S = _ref(c)
    y = _standin(c)
    y[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_bf16_close(y, ref, S, c["K"])
    with pytest.raises(AssertionError):
        assert_bf16_close(_standin(c)[:, 1:], ref, S, c["K"])
    with pytest.raises(ValueError):
        conv_ref64(c["x"], c["wp"], act="silu")
