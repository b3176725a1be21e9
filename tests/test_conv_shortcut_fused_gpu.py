"""Implicit-GEMM conv with extra K segments (csk_conv2d_ex2 / csk_conv2d_gn2:
a ResNet's 1x1 shortcut folded into its conv2's K loop), each output element
against the float64 reference

    conv_ref64(h, wp, bias) + a . Wa^T + b . Wb^T

within the per-element bf16 bound of tests/_numerics.py at K = 9 Cin + Ca + Cb
(S: the same expression on absolute values).

Shapes: B = 2, 9x7 (126 rows: ragged against every BM, two samples in one
tile) and one B = 3, 8x8; Cin 64 / 128; segments (64,), (128, 64), (64, 192);
Cout 48 (ragged N edge) / 176 (a second, ragged column tile at 160 wide).
Splits 1, 3, 4: at Cin = 64 with (128, 64), K = 768 = 12 K-steps, split 3 puts
tap 8 and both segments into the last split and split 4 makes the last split
segment-only, starting exactly on the tap-to-segment boundary; at Cin = 128
split 3 starts inside the tap range with the segments following.

Every operand the kernel gathers (x and each source) is a channel-slice view
of a wider NHWC buffer whose other channels are NaN, and the output starts as
NaN: a read outside a slice or an unwritten element fails the bound.

Tiles 26 / 11 / 14 (gemm_glds_kernel), 33 (gemm8r_kernel).  The phased kernel
(tile 31) and the register-staged tiles (1) are not extended: the entry point
must refuse them."""
import functools
import math

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.ops import hip_ops
from tests._numerics import assert_bf16_close, conv_ref64

pytestmark = pytest.mark.gpu

TILES = (26, 11, 14, 33)
SPLITS = (1, 3, 4)
SEGS = ((64,), (128, 64), (64, 192))
CASES = [(2, 9, 7, cin, segs, cout) for cin in (64, 128) for segs in SEGS for cout in (48, 176)]
CASES.append((3, 8, 8, 64, (128, 64), 176))
PAD_LEFT, PAD_RIGHT = 8, 16  # NaN channels around every slice (16-byte aligned slices, pixel stride % 8 == 0)


def _ids(c):
    B, H, W, cin, segs, cout = c
    return f"B{B}-{H}x{W}-C{cin}-x{'_'.join(map(str, segs))}-N{cout}"


@functools.lru_cache(maxsize=None)
def _case(B, H, W, cin, segs, cout):
    """bf16 operands (CPU, seeded), the fused weight, and the float64 reference; computed once and shared."""
    g = torch.Generator().manual_seed(B * 100000 + H * 1000 + cin * 7 + sum(segs) * 3 + cout + len(segs))
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16)  # noqa: E731
    K = 9 * cin + sum(segs)
    c = dict(x=r(B, H, W, cin), wp=r(cout, 3, 3, cin, scale=K ** -0.5), bias=r(cout),
             src=[r(B, H, W, ci) for ci in segs], ws=[r(cout, ci, scale=K ** -0.5) for ci in segs])
    ref, S = conv_ref64(c["x"], c["wp"], c["bias"], 1, 1)
    for a, wa in zip(c["src"], c["ws"]):
        a64, w64 = a.double(), wa.double()
        ref = ref + a64 @ w64.t()
        S = S + a64.abs() @ w64.abs().t()
    wf = torch.cat([c["wp"].reshape(cout, -1)] + c["ws"], 1).contiguous()
    c.update(ref=ref, S=S, K=K, wf=wf)
    return c


def _slice_of_wide(t, dev):
    """``t`` as a channel-slice view of a wider NHWC buffer, NaN everywhere else"""
    B, H, W, C = t.shape
    wide = torch.full((B, H, W, PAD_LEFT + C + PAD_RIGHT), float("nan"), dtype=torch.bfloat16, device=dev)
    wide[..., PAD_LEFT:PAD_LEFT + C] = t.to(dev)
    v = wide[..., PAD_LEFT:PAD_LEFT + C]
    assert v.data_ptr() % 16 == 0 and hip_ops._pix_stride(v) % 8 == 0 and hip_ops._pix_stride(v) > C
    return v


def _seg_args(srcs):
    from chiaswarm_amd.ops.hip_ops import _p, _pix_stride

    a = srcs[0]
    b = srcs[1] if len(srcs) > 1 else None
    return (_p(a), _pix_stride(a), a.shape[3], _p(b), _pix_stride(b) if b is not None else 0,
            b.shape[3] if b is not None else 0)


def _conv_ex2(tile, split, x, wf, bias, srcs, out, part=None):
    """csk_conv2d_ex2 (3x3, stride 1, pad 1) with an explicit tile and split on the views it is given"""
    from chiaswarm_amd.ops import _lib
    from chiaswarm_amd.ops.hip_ops import _p, _pix_stride, _s

    B, H, W, Cin = x.shape
    Cout = wf.shape[0]
    assert wf.is_contiguous() and wf.shape[1] == 9 * Cin + sum(s.shape[3] for s in srcs)
    M = B * H * W
    ws = torch.empty(split * M * Cout, dtype=torch.float32, device=x.device) if split > 1 else None
    _lib.call("csk_conv2d_ex2", _p(out), _p(x), _p(wf), _p(bias), None, 0, None, B, H, W, Cin, Cout, 3, 3, 1, 1, 1,
              H, W, 0, _pix_stride(x), _pix_stride(out), 0, 0, 1.0, 1, _p(part), tile, split, _p(ws),
              *_seg_args(srcs), _s())


def _device_case(c, dev):
    if "dev" not in c:
        c["dev"] = dict(x=_slice_of_wide(c["x"], dev), src=[_slice_of_wide(a, dev) for a in c["src"]],
                        wf=c["wf"].to(dev), bias=c["bias"].to(dev))
    return c["dev"]


@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("tile", TILES)
def test_conv_extra_segments_by_tile(gpu, tile, case):
    B, H, W, cin, segs, cout = case
    c = _case(*case)
    d = _device_case(c, gpu)
    for split in SPLITS:
        out = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=gpu)  # unwritten stays NaN
        _conv_ex2(tile, split, d["x"], d["wf"], d["bias"], d["src"], out)
        worst = assert_bf16_close(out, c["ref"], c["S"], c["K"], f"tile {tile} {_ids(case)} split={split}",
                                  tag="gemm8p" if tile == 33 else "gemm_glds")
        print(f"tile {tile} {_ids(case)} split={split}: worst |y - ref| / tol = {worst:.3f}")


@pytest.mark.parametrize("tile", [31, 1, 0])
@pytest.mark.parametrize("split", [1, 3])
def test_unextended_kernels_are_refused(gpu, tile, split):
    """The phased 8-wave kernel and the register-staged tiles do not walk
    segments: an error, never a silent run of the plain conv."""
    case = (2, 9, 7, 64, (128, 64), 48)
    c = _case(*case)
    d = _device_case(c, gpu)
    out = torch.full((2, 9, 7, 48), float("nan"), dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError, match="hipError"):
        _conv_ex2(tile, split, d["x"], d["wf"], d["bias"], d["src"], out)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all(), "a refused call wrote its output"


def test_conditions_are_refused(gpu):
    """Geometry the segment walk does not cover is an error of the entry point:
    the in-kernel fixup split, a source pixel stride that is not a multiple of
    8, a misaligned source, a channel count that is no multiple of 64."""
    from chiaswarm_amd.ops import _lib
    from chiaswarm_amd.ops.hip_ops import _p, _s

    case = (2, 9, 7, 64, (128, 64), 48)
    c = _case(*case)
    d = _device_case(c, gpu)
    out = torch.full((2, 9, 7, 48), float("nan"), dtype=torch.bfloat16, device=gpu)
    a, b = d["src"]
    ws = torch.empty(4 * (126 + 255) * (48 + 255), dtype=torch.float32, device=gpu)

    def call(split=1, a_ld=None, a_ptr=None, ca=128, stride=1):
        _lib.call("csk_conv2d_ex2", _p(out), _p(d["x"]), _p(d["wf"]), _p(d["bias"]), None, 0, None, 2, 9, 7, 64, 48,
                  3, 3, stride, 1, 1, 9, 7, 0, hip_ops._pix_stride(d["x"]), 48, 0, 0, 1.0, 1, None, 11, split, _p(ws),
                  a_ptr or _p(a), a_ld or hip_ops._pix_stride(a), ca, _p(b), hip_ops._pix_stride(b), 64, _s())

    for kw in (dict(split=-3), dict(a_ld=hip_ops._pix_stride(a) + 4), dict(a_ptr=a.data_ptr() + 2), dict(ca=96),
               dict(stride=2)):
        with pytest.raises(RuntimeError, match="hipError"):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()


def bf16_step(mag: float) -> float:
    """spacing of bf16 values (8 significant bits) at magnitude ``mag``"""
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - 7)


def _gn64(y, gamma, beta, groups, eps, silu):
    B, H, W, C = y.shape
    v = y.reshape(B, H * W, groups, C // groups)
    mean = v.mean(dim=(1, 3), keepdim=True)
    var = v.var(dim=(1, 3), unbiased=False, keepdim=True)
    o = ((v - mean) / torch.sqrt(var + eps)).reshape(B, H, W, C) * gamma + beta
    return o * torch.sigmoid(o) if silu else o


@pytest.mark.parametrize("keep_raw", [True, False])
def test_conv_extra_segments_fused_reduce_group_norm(gpu, keep_raw):
    """csk_conv2d_gn2, tile 33, split 3, 32 groups + SiLU, against the float64
    GroupNorm of the float64 reference.  Tolerance: the rule of
    tests/test_splitk_gn_fused_gpu.py: the fused reduce + apply and the unfused
    pair (the same split conv, then ``group_norm``) share the raw fp32 value and
    round once, so the fused error is at most the unfused error plus one bf16
    step at the largest output magnitude; the kept raw output is bit-identical."""
    from chiaswarm_amd.ops import _lib
    from chiaswarm_amd.ops.hip_ops import _p, _pix_stride, _s

    case = (2, 9, 7, 64, (128, 64), 128)
    B, H, W, cin, segs, cout = case
    groups, eps = 32, 1e-5
    c = _case(*case)
    d = _device_case(c, gpu)
    g = torch.Generator().manual_seed(77)
    gamma = (torch.randn(cout, generator=g) * 0.3 + 1.0).to(torch.bfloat16)
    beta = (torch.randn(cout, generator=g) * 0.5).to(torch.bfloat16)
    ref = _gn64(c["ref"], gamma.double(), beta.double(), groups, eps, True)
    gd, bd = gamma.to(gpu), beta.to(gpu)
    # unfused: the split conv's raw output, then the GroupNorm kernel
    raw_u = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=gpu)
    _conv_ex2(33, 3, d["x"], d["wf"], d["bias"], d["src"], raw_u)
    unf = hip_ops.group_norm(raw_u, gd, bd, groups, eps, True)
    # fused
    raw = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=gpu)
    yn = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=gpu)
    M = B * H * W
    ws = torch.empty(3 * M * cout, dtype=torch.float32, device=gpu)
    _lib.call("csk_conv2d_gn2", _p(raw) if keep_raw else None, _p(d["x"]), _p(d["wf"]), _p(d["bias"]), None, 0, None,
              B, H, W, cin, cout, 3, 3, 1, 1, 1, H, W, 0, _pix_stride(d["x"]), cout, 0, 1.0, 1, 33, 3, _p(ws), _p(yn),
              _p(gd), _p(bd), groups, eps, 1, int(keep_raw), *_seg_args(d["src"]), _s())
    e_unf = (unf.double().cpu() - ref).abs().max().item()
    e_fus = (yn.double().cpu() - ref).abs().max().item()
    bound = e_unf + bf16_step(ref.abs().max().item())
    print(f"keep_raw={keep_raw}: fused err {e_fus:.5f}, unfused {e_unf:.5f}, bound {bound:.5f}")
    assert math.isfinite(e_fus) and e_fus <= bound
    if keep_raw:
        assert torch.equal(raw, raw_u), "raw conv output not bit-identical to the unfused split conv's"
        assert_bf16_close(raw, c["ref"], c["S"], c["K"], "csk_conv2d_gn2 raw output")
    else:
        assert torch.isnan(raw.float()).all()


@pytest.mark.parametrize("tile", [26, 33])
def test_conv_extra_segments_epilogue_statistics(gpu, tile):
    """``gn_stats=True`` through ``hip_ops.conv2d(extra=...)``: the statistics the
    epilogue attaches are the mean and M2 of the output it stored (tolerances of
    tests/test_kernels_gpu.py test_fused_group_norm_stats_split_k)."""
    from chiaswarm_amd.ops import tuning

    B, H, W, cin, segs, cout = 2, 16, 16, 64, (128, 64), 160
    c = _case(B, H, W, cin, segs, cout)
    d = _device_case(c, gpu)
    _, wv, wsv = ops.pack_conv_extra(c["wp"].to(gpu), [w.to(gpu) for w in c["ws"]])
    extra = tuple(zip(d["src"], wsv))
    assert hip_ops.conv_extra_ok(d["x"], wv, extra)
    key = f"c:{B}:{H}:{W}:{cin}:{cout}:3:1:0:x128:64"
    t = tuning.table()
    old = t.get(key)
    t[key] = [tile, 1, 0.0]
    try:
        n0 = hip_ops.SC_FUSE_STATS[0]
        y = hip_ops.conv2d(d["x"], wv, d["bias"], 1, 1, None, False, None, gn_stats=True, extra=extra)
        assert hip_ops.SC_FUSE_STATS[0] == n0 + 1
    finally:
        if old is None:
            t.pop(key, None)
        else:
            t[key] = old
    assert_bf16_close(y, c["ref"], c["S"], c["K"], f"tile {tile} with statistics")
    assert getattr(y, "_csk_gn", None) is not None
    part, seg = y._csk_gn
    yv = y.float().reshape(-1, seg, cout)
    pm = part.view(-1, cout, 2)
    assert torch.allclose(pm[..., 0], yv.mean(1), atol=2e-2)
    m2 = yv.var(1, unbiased=False) * seg
    assert ((pm[..., 1] - m2).norm() / m2.norm()).item() < 2e-2
