"""Split-K conv whose reduce kernel also applies the GroupNorm (+ SiLU) that
consumes its output (gemm.hip splitk_reduce_gn_apply_kernel, reached through
``conv2d(..., norm=...)``), against an fp32 CPU conv -> bias / time bias /
residual -> GroupNorm -> SiLU, with the unfused pair of kernels (switch off,
same inputs) as the yardstick.

Error bound (not a constant): the fused and the unfused path share the raw
fp32 value and round once at the end, so they can differ only where the order
of the fp32 additions in the statistics moves a value across a bf16 rounding
boundary.  The fused output's error against the fp32 reference is therefore at
most the unfused path's error plus one bf16 rounding step at the largest
output magnitude."""
import dataclasses
import itertools
import math

import pytest
import torch

from chiaswarm_amd import ops
from chiaswarm_amd.ops import hip_ops, tuning

pytestmark = pytest.mark.gpu

GROUPS, EPS, CIN = 32, 1e-5, 128


class _Force:
    def __init__(self, keys, tile, split):
        self.keys, self.tile, self.split = keys, tile, split

    def __enter__(self):
        t = tuning.table()
        self.old = {k: t.get(k) for k in self.keys}
        for k in self.keys:
            t[k] = [self.tile, self.split, 0.0]

    def __exit__(self, *exc):
        t = tuning.table()
        for k, v in self.old.items():
            if v is None:
                t.pop(k, None)
            else:
                t[k] = v


class _Switch:
    """the fused kernel on / off, restored on exit.  These shapes are the smallest
    that reach every branch, 64 / 96 workgroups, so like the tile and the split the
    grid floor below which the host keeps two kernels is forced (``min_wg``; None
    leaves the library's default)."""

    def __init__(self, on, min_wg=0):
        self.on, self.min_wg = on, min_wg

    def __enter__(self):
        self.old = hip_ops.SKGN_FUSED
        hip_ops.set_skgn_fused(self.on)
        self.old_wg = hip_ops.set_skgn_min_wg(self.min_wg) if self.min_wg is not None else None

    def __exit__(self, *exc):
        hip_ops.set_skgn_fused(self.old)
        if self.old_wg is not None:
            hip_ops.set_skgn_min_wg(self.old_wg)


def bf16_step(mag: float) -> float:
    """spacing of bf16 values (8 significant bits) at magnitude ``mag``"""
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - 7)


def rnd(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


_CASES = {}


def _case(B, H, Cout):
    """Inputs of one shape (CPU bf16 masters + device copies) and the fp32 conv
    of them, computed once and shared by every test of that shape."""
    key = (B, H, Cout)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * B + 10 * H + Cout)
        c = {
            "x": rnd(B, H, H, CIN, g=g),
            "wp": ops.pack_conv_weight(rnd(Cout, CIN, 3, 3, g=g, scale=(9 * CIN) ** -0.5)),
            "bias": rnd(Cout, g=g),
            "b2wide": rnd(B, 3 * Cout + 8, g=g),       # bias2d = a strided column slice of this
            "reswide": rnd(B, H, H, 2 * Cout, g=g),   # residual = a channel-slice view of this
            "gamma": (torch.randn(Cout, generator=g) * 0.3 + 1.0).to(torch.bfloat16),
            "beta": rnd(Cout, g=g, scale=0.5),
        }
        c["conv32"] = ops._ref_conv2d(c["x"].float(), c["wp"].float(), None, 1, 1, None, False, None)
        _CASES[key] = c
    return _CASES[key]


def _dev(c, name, dev):
    k = name + "@dev"
    if k not in c:
        c[k] = c[name].to(dev)
    return c[k]


def _reference(c, bias, b2, res, silu, Cout, out_scale=1.0):
    y = c["conv32"]
    if bias:
        y = y + c["bias"].float()
    if b2:
        y = y + c["b2wide"][:, Cout:2 * Cout].float()[:, None, None, :]
    if out_scale != 1.0:
        y = y * out_scale
    if res:
        y = y + c["reswide"][..., Cout:].float()
    return ops._ref_group_norm(y, c["gamma"].float(), c["beta"].float(), GROUPS, EPS, silu)


def _run(c, dev, Cout, bias, b2, res, silu, keep_raw, out_scale=1.0):
    got = hip_ops.conv2d(_dev(c, "x", dev), _dev(c, "wp", dev), _dev(c, "bias", dev) if bias else None, 1, 1,
                         _dev(c, "reswide", dev)[..., Cout:] if res else None, False,
                         _dev(c, "b2wide", dev)[:, Cout:2 * Cout] if b2 else None, out_scale=out_scale,
                         norm=(_dev(c, "gamma", dev), _dev(c, "beta", dev), GROUPS, EPS, silu, keep_raw))
    return got if keep_raw else (got, None)


# (B, H = W, Cout): 8x8 / 4x4 and the ragged 6x6 (36 px per sample, M = 108 against
# every tile and segment); Cout / 32 groups = 4, 20, 40 channels per group (fused)
# and 2 (not a multiple of 4: must fall back and still be right)
SHAPES = [(2, 8, 128), (3, 6, 128), (2, 8, 640), (3, 6, 640), (2, 4, 1280), (2, 8, 64), (3, 6, 64)]


@pytest.mark.parametrize("split", [2, 4, 16])
@pytest.mark.parametrize("B,H,Cout", SHAPES)
def test_fused_reduce_gn(gpu, B, H, Cout, split):
    c = _case(B, H, Cout)
    eligible = (Cout // GROUPS) % 4 == 0
    key = f"c:{B}:{H}:{H}:{CIN}:{Cout}:3:1:0"
    worst = 0.0
    with _Force([key], 11, split):
        for bias, b2, res, silu, keep_raw in itertools.product([False, True], repeat=5):
            ref = _reference(c, bias, b2, res, silu, Cout)
            with _Switch(False):
                n0 = list(hip_ops.SKGN_STATS)
                unf, unf_raw = _run(c, gpu, Cout, bias, b2, res, silu, True)
                assert hip_ops.SKGN_STATS[0] == n0[0] and hip_ops.SKGN_STATS[1] == n0[1] + 1
            with _Switch(True):
                n0 = list(hip_ops.SKGN_STATS)
                fus, fus_raw = _run(c, gpu, Cout, bias, b2, res, silu, keep_raw)
                assert hip_ops.SKGN_STATS[0] == n0[0] + int(eligible), "fused counter"
                assert hip_ops.SKGN_STATS[1] == n0[1] + int(not eligible), "fallback counter"
            e_unf = (unf.float().cpu() - ref).abs().max().item()
            e_fus = (fus.float().cpu() - ref).abs().max().item()
            bound = e_unf + bf16_step(ref.abs().max().item())
            worst = max(worst, e_fus / bound)
            tag = (bias, b2, res, silu, keep_raw)
            assert e_fus <= bound, f"{tag}: fused err {e_fus:.5f} > unfused {e_unf:.5f} + one bf16 step"
            if keep_raw:
                assert torch.equal(fus_raw, unf_raw), f"{tag}: raw conv output not bit-identical"
            if not eligible:
                assert torch.equal(fus, unf)
    print(f"B={B} {H}x{H} Cout={Cout} split={split}: worst fused err / bound = {worst:.3f}")


@pytest.mark.parametrize("tile", [4, 33])
def test_fused_reduce_gn_other_tiles_and_out_scale(gpu, tile):
    """The register-staged and the 8-wave conv kernels feed the same reduce; an
    output scale sits between the time bias and the residual."""
    B, H, Cout = 3, 6, 640
    c = _case(B, H, Cout)
    ref = _reference(c, True, True, True, True, Cout, out_scale=0.5)
    with _Force([f"c:{B}:{H}:{H}:{CIN}:{Cout}:3:1:0"], tile, 4):
        with _Switch(False):
            unf, unf_raw = _run(c, gpu, Cout, True, True, True, True, True, out_scale=0.5)
        with _Switch(True):
            n0 = hip_ops.SKGN_STATS[0]
            fus, fus_raw = _run(c, gpu, Cout, True, True, True, True, True, out_scale=0.5)
            assert hip_ops.SKGN_STATS[0] == n0 + 1
    e_unf = (unf.float().cpu() - ref).abs().max().item()
    e_fus = (fus.float().cpu() - ref).abs().max().item()
    assert e_fus <= e_unf + bf16_step(ref.abs().max().item())
    assert torch.equal(fus_raw, unf_raw)


# One thread finishes items t, t + 1024, ...: the shapes above are at most 320
# items per workgroup, one item per thread.  These reach 2, 3, 4 and 5 items per
# thread (the kernel instances the UNet step runs: 5 at 32x32 x 640, 3 at 16x16 x
# 1280), most with a ragged last slot (threads whose last item does not exist).
# (H = W, Cout, split, items = H * W * Cout / 32 / 4, items per thread)
MULTI = [(32, 640, 2, 5120, 5), (16, 1280, 4, 2560, 3), (24, 640, 4, 2880, 3), (30, 640, 2, 4500, 5),
         (20, 640, 16, 2000, 2), (28, 640, 16, 3920, 4), (16, 640, 4, 1280, 2)]
MULTI_VARIANTS = [  # (bias, bias2d, residual, silu, keep_raw): each on and off, both ways with keep_raw
    (False, False, False, False, False), (True, True, True, True, True), (True, False, True, False, False),
    (False, True, False, True, True), (True, True, False, True, False), (False, False, True, False, True)]


class _Unroll:
    """splits loaded per memory round trip in the split-K reduces (csk_set_skr_unroll), restored on exit"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from chiaswarm_amd.ops import _lib

        self.old = _lib.call_int("csk_get_skr_unroll")
        _lib.call("csk_set_skr_unroll", self.n)

    def __exit__(self, *exc):
        from chiaswarm_amd.ops import _lib

        _lib.call("csk_set_skr_unroll", self.old)


@pytest.mark.parametrize("unroll", [4, 1])
@pytest.mark.parametrize("H,Cout,split,items,ipt", MULTI)
def test_fused_reduce_gn_several_items_per_thread(gpu, H, Cout, split, items, ipt, unroll):
    """Same bound, bit-identical raw output and counters as above, at 2-5 items
    per thread, with 4 / 2 (unroll 4) and 1 (unroll 1) splits per round trip."""
    B = 2
    assert items == H * H * (Cout // GROUPS // 4) and ipt == -(-items // 1024)
    c = _case(B, H, Cout)
    worst = 0.0
    with _Force([f"c:{B}:{H}:{H}:{CIN}:{Cout}:3:1:0"], 11, split), _Unroll(unroll):
        for bias, b2, res, silu, keep_raw in MULTI_VARIANTS:
            ref = _reference(c, bias, b2, res, silu, Cout)
            with _Switch(False):
                unf, unf_raw = _run(c, gpu, Cout, bias, b2, res, silu, True)
            with _Switch(True):
                n0 = list(hip_ops.SKGN_STATS)
                fus, fus_raw = _run(c, gpu, Cout, bias, b2, res, silu, keep_raw)
                assert hip_ops.SKGN_STATS == [n0[0] + 1, n0[1], n0[2]], "fused counter"
            e_unf = (unf.float().cpu() - ref).abs().max().item()
            e_fus = (fus.float().cpu() - ref).abs().max().item()
            bound = e_unf + bf16_step(ref.abs().max().item())
            worst = max(worst, e_fus / bound)
            tag = (bias, b2, res, silu, keep_raw)
            assert e_fus <= bound, f"{tag}: fused err {e_fus:.5f} > unfused {e_unf:.5f} + one bf16 step"
            if keep_raw:
                assert torch.equal(fus_raw, unf_raw), f"{tag}: raw conv output not bit-identical"
    print(f"{H}x{H} Cout={Cout} split={split} ({items} items, {ipt} per thread) unroll={unroll}: "
          f"worst fused err / bound = {worst:.3f}")


def test_fused_reduce_gn_ineligible_plans(gpu):
    """No split, the in-kernel fixup split and a per-sample affine are not the
    reduce kernel's: conv + GroupNorm, counted as fallbacks."""
    B, H, Cout = 2, 8, 128
    c = _case(B, H, Cout)
    key = f"c:{B}:{H}:{H}:{CIN}:{Cout}:3:1:0"
    ref = _reference(c, True, False, False, True, Cout)

    def rel_err(y):  # the bound tests/test_gemm_fixup_gpu.py holds this conv -> GroupNorm pair to
        return ((y.float().cpu() - ref).norm() / ref.norm()).item()

    for tile, split in ((11, 1), (14, -4)):
        with _Force([key], tile, split):
            with _Switch(False):
                off, _ = _run(c, gpu, Cout, True, False, False, True, False)
            with _Switch(True):
                n0 = list(hip_ops.SKGN_STATS)
                y, _ = _run(c, gpu, Cout, True, False, False, True, False)
                assert hip_ops.SKGN_STATS == [n0[0], n0[1] + 1, n0[2]]
        assert torch.equal(y, off) and rel_err(y) < 1e-2
    with _Force([key], 11, 4):  # 2 x 32 workgroups: under the default grid floor, fused with the floor at 64
        for min_wg, fused in ((None, 0), (64, 1), (65, 0)):
            with _Switch(True, min_wg):
                n0 = list(hip_ops.SKGN_STATS)
                y, _ = _run(c, gpu, Cout, True, False, False, True, False)
                assert hip_ops.SKGN_STATS == [n0[0] + fused, n0[1] + 1 - fused, n0[2]]
            assert rel_err(y) < 1e-2
        with _Switch(False):  # norm_optional: the raw output with its statistics, the norm left to the consumer
            n0 = list(hip_ops.SKGN_STATS)
            yn, raw = hip_ops.conv2d(_dev(c, "x", gpu), _dev(c, "wp", gpu), _dev(c, "bias", gpu), 1, 1, None, False,
                                     None, norm=(_dev(c, "gamma", gpu), _dev(c, "beta", gpu), GROUPS, EPS, True, True),
                                     norm_optional=True)
            assert yn is None and getattr(raw, "_csk_gn", None) is not None
            assert hip_ops.SKGN_STATS == [n0[0], n0[1], n0[2] + 1]
    with pytest.raises(ValueError):  # out= is the raw output's buffer: meaningless unless the raw output is kept
        hip_ops.conv2d(_dev(c, "x", gpu), _dev(c, "wp", gpu), None, 1, 1, None, False, None,
                       out=torch.empty(B, H, H, Cout, dtype=torch.bfloat16, device=gpu),
                       norm=(_dev(c, "gamma", gpu), _dev(c, "beta", gpu), GROUPS, EPS, True, False))
    g2 = _dev(c, "gamma", gpu)[None].expand(B, Cout).contiguous()
    b2 = _dev(c, "beta", gpu)[None].expand(B, Cout).contiguous()
    with _Force([key], 11, 4), _Switch(True):
        n0 = list(hip_ops.SKGN_STATS)
        y = hip_ops.conv2d(_dev(c, "x", gpu), _dev(c, "wp", gpu), _dev(c, "bias", gpu), 1, 1, None, False, None,
                           norm=(g2, b2, GROUPS, EPS, True, False))
        assert hip_ops.SKGN_STATS == [n0[0], n0[1] + 1, n0[2]]
    assert rel_err(y) < 1e-2


def test_fused_reduce_gn_graph_replay(gpu):
    """Captured in a hipGraph and replayed twice with another split-K conv (its
    own fp32 workspace traffic) in between: both replays bitwise equal."""
    B, H, Cout = 2, 8, 640
    c = _case(B, H, Cout)
    o = _case(3, 6, 128)
    keys = [f"c:{B}:{H}:{H}:{CIN}:{Cout}:3:1:0", f"c:3:6:6:{CIN}:128:3:1:0"]
    with _Force(keys, 11, 4), _Switch(True):
        eager, eager_raw = _run(c, gpu, Cout, True, True, True, True, True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _run(c, gpu, Cout, True, True, True, True, True)
        torch.cuda.current_stream().wait_stream(s)
        n0 = hip_ops.SKGN_STATS[0]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            yn, raw = _run(c, gpu, Cout, True, True, True, True, True)
        assert hip_ops.SKGN_STATS[0] == n0 + 1
        g.replay()
        torch.cuda.synchronize()
        first, first_raw = yn.clone(), raw.clone()
        other, _ = _run(o, gpu, 128, True, False, False, False, False)
        yn.zero_()
        raw.zero_()
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(yn, first) and torch.equal(raw, first_raw)
    assert torch.equal(first, eager) and torch.equal(first_raw, eager_raw)
    assert torch.isfinite(other.float()).all()


def _tiny_unet_pair(gpu, cfg, seed):
    from chiaswarm_amd.models import unet as unet_mod
    from chiaswarm_amd.models.layers import init_random_, prepare_model

    m = unet_mod.UNet2DConditionModel(cfg).eval()
    init_random_(m, seed=seed)
    m = m.to(torch.bfloat16)
    twin = unet_mod.UNet2DConditionModel(cfg).eval()
    twin.load_state_dict({k: v.float() for k, v in m.state_dict().items()})  # fp32 twin of the bf16 weights
    return prepare_model(m.to(gpu)), prepare_model(twin)


def _force_split_convs(monkeypatch):
    """every 3x3 conv with at least four 64-wide K steps runs split in two"""
    real = tuning.choose

    def choose(key, M, N, K, runner):
        if key.startswith("c:") and K >= 256 and N >= 32:
            return 18, 2
        return real(key, M, N, K, runner)

    monkeypatch.setattr(tuning, "choose", choose)


@torch.no_grad()
def test_tiny_unet_step_fused_vs_unfused(gpu, monkeypatch):
    """One step of the tiny UNet family with the switch on and off, its 3x3 convs
    forced to split K.  The family's widths (32 / 64) with 32 groups give 1 / 2
    channels per group, which the fused kernel does not take (fp32x4 loads): that
    configuration must run all-fallback and bit-identical; with 8 groups (4 / 8
    channels per group, same topology) the ResNet sites fuse.

    Bound, propagated: a fused site changes an activation by at most one bf16
    rounding step (the test above), i.e. by no more than the roundings the bf16
    path already makes at every layer, and it is the accumulation of exactly those
    roundings that separates the unfused step from its fp32 twin.  So the fused
    and the unfused step may differ by at most the unfused step's error against
    the fp32 twin plus one bf16 step at the largest output magnitude."""
    from chiaswarm_amd.models import unet as unet_mod

    _force_split_convs(monkeypatch)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 8, 8, 4, generator=g)
    ctx = torch.randn(2, 7, 32, generator=g)
    t = torch.tensor([500.0])
    for groups, want_fused in ((8, True), (32, False)):
        cfg = dataclasses.replace(unet_mod.TINY, norm_num_groups=groups)
        m, twin = _tiny_unet_pair(gpu, cfg, seed=5)
        ref = twin(x, t, encoder_hidden_states=ctx)
        xg, cg, tg = x.to(gpu, torch.bfloat16), ctx.to(gpu, torch.bfloat16), t.to(gpu)
        with _Switch(False):
            n0 = list(hip_ops.SKGN_STATS)
            off = m(xg, tg, encoder_hidden_states=cg).float().cpu()
            assert hip_ops.SKGN_STATS[0] == n0[0]
            sites = sum(hip_ops.SKGN_STATS[1:]) - sum(n0[1:])
        with _Switch(True):
            n0 = list(hip_ops.SKGN_STATS)
            on = m(xg, tg, encoder_hidden_states=cg).float().cpu()
            fused = hip_ops.SKGN_STATS[0] - n0[0]
        e_off = (off - ref).abs().max().item()
        d = (on - off).abs().max().item()
        print(f"groups={groups}: {fused} of {sites} conv+norm sites fused, |on - off| {d:.5f}, "
              f"unfused vs fp32 twin {e_off:.5f}, max |ref| {ref.abs().max().item():.3f}")
        assert sites > 0
        if want_fused:
            assert fused > 0, "no conv + GroupNorm site took the fused reduce"
            assert d <= e_off + bf16_step(ref.abs().max().item())
        else:
            assert fused == 0 and torch.equal(on, off)


@pytest.mark.parametrize("plan,fused", [((11, 4), True), ((11, 1), False)])
def test_norm_without_raw_when_choose_times_plans(gpu, monkeypatch, plan, fused):
    """``tuning.choose`` may launch ``runner(tile, split)`` for every candidate plan
    (CSK_AUTOTUNE=1 on a table miss) before conv2d knows whether the reduce will
    apply the norm: with ``norm`` and no ``keep_raw`` the runner must still write a
    real raw buffer, whichever plan is then chosen."""
    from chiaswarm_amd.ops import _lib

    B, H, Cout = 2, 8, 128
    c = _case(B, H, Cout)
    ref = _reference(c, True, False, False, True, Cout)
    seen = []
    real_call = _lib.call

    def call(name, *args):
        if name == "csk_conv2d_ex":
            seen.append(args[0])  # Y
        return real_call(name, *args)

    def choose(key, M, N, K, runner):
        for tile, split in ((11, 1), (4, 2), (11, 4)):
            runner(tile, split)
        return plan

    monkeypatch.setattr(tuning, "choose", choose)
    monkeypatch.setattr(hip_ops._lib, "call", call)
    with _Switch(True):
        n0 = list(hip_ops.SKGN_STATS)
        y, _ = _run(c, gpu, Cout, True, False, False, True, False)
        assert hip_ops.SKGN_STATS == [n0[0] + int(fused), n0[1] + int(not fused), n0[2]]
    assert len(seen) == (3 if fused else 4) and all(seen), f"raw output pointers the conv launcher saw: {seen}"
    assert ((y.float().cpu() - ref).norm() / ref.norm()).item() < 1e-2
    with pytest.raises(RuntimeError):  # the launcher itself refuses a null output
        real_call("csk_conv2d_ex", None, _dev(c, "x", gpu).data_ptr(), _dev(c, "wp", gpu).data_ptr(), None, None, 0,
                  None, B, H, H, CIN, Cout, 3, 3, 1, 1, 1, H, H, 0, CIN, Cout, 0, 0, 1.0, 1, None, 11, 1, None,
                  hip_ops._s())
