"""The K-partitioned split-bf16 conv tiles (plan tiles 17 and 18: csrc/conv_gemm_glds.inc, WGK = 2).

The block's four waves are 2 (M) x 1 (N) x 2 (K): a wave multiplies its 64- (32-) row x 64-column sub-tile over ONE of the two
16-k pairs of every 32-deep chunk, and after the K loop the two waves of a pair of k halves exchange half of their accumulators
through LDS and add, so that the shared epilogue sees the layout of 2 x 2 waves.  What can go wrong is the exchange (which
column goes where, the LDS area it overlays, its barriers against the operand DMA of this and of the next M tile) and the
place of a wave's pair in the chunk -- so the cases are the smallest shapes that reach each of these: one chunk per tap,
an odd number of chunks, ragged row and column tiles, split reductions with uneven and empty ranges, a persistent M loop.

Truth is torch's fp64 convolution of the same fp32 operands (wide-range values: random signs, magnitudes over 2^+-12, a block
of exact zeros -- the generator of test_f32_products_on_the_bf16_pipe).  Criterion, the one that test uses: the rel-L2 error
is at most 1.05 x that of the fp32-MFMA tile of the same block shape (13 for 17, 14 for 18) on the same inputs and plan split,
and below 2e-6.  Statistics, bwd_sums and the residual mix: the tolerances of test_conv_lds_dma_tiles against the fp32
emulation."""
import functools
import math

import pytest
import torch

import torch_backend as TB
from mimic_amd import ops
from mimic_amd.ops import Geom, Mask
from test_hip_ops_gpu import DEV, _err64, _log, check, make_bn, to_dev

pytestmark = pytest.mark.gpu

KPART = ((17, 13), (18, 14))      # (K-partitioned tile, fp32-MFMA tile of the same block shape)

GEOMS = {
    # 1x1, 40 rows (under one block, not a multiple of 32).  fwd: Ck = 32 -> ONE chunk, Cn = 96 -> ragged last column tile;
    # dgrad: Ck = 96 -> three chunks, Cn = 32
    "c1x1_32to96_r40": Geom(1, 5, 8, 5, 8, 32, 96, 1, 1, 1, 1, 0, 0, False),
    # the mirror image: fwd three chunks / Cn = 32, dgrad one chunk / Cn = 96
    "c1x1_96to32_r40": Geom(1, 5, 8, 5, 8, 96, 32, 1, 1, 1, 1, 0, 0, False),
    # transposed 1x1, 90 rows.  fwd: Ck = 128 -> four chunks (split 3: ranges 2, 2, 0 -- an EMPTY one), Cn = 64; dgrad: two chunks
    "t1x1_128to64_r90": Geom(2, 5, 9, 5, 9, 128, 64, 1, 1, 1, 1, 0, 0, True),
    # transposed k4 s2 on an odd grid, 60 rows per phase.  fwd: 4 taps x 3 chunks = 12 per phase (split 5: 3, 3, 3, 3, 0);
    # dgrad: 16 taps x 1 chunk (split 3: 6, 6, 4)
    "t_k4s2_96to32_odd": Geom(2, 5, 6, 10, 12, 96, 32, 4, 4, 2, 2, 1, 1, True),
    # conv k4 s2, 48 rows.  fwd: 16 taps x 2 chunks, Cn = 96; dgrad: 4 taps x 3 chunks per phase
    "c_k4s2_64to96": Geom(3, 4, 4, 8, 8, 64, 96, 4, 4, 2, 2, 1, 1, False),
}
# the persistent M loop: 4096 rows per phase, four phases, plan split 8 -> 512 / (4 x 8) = 16 blocks walk the 32 (tile 17) or
# 64 (tile 18) M tiles of a phase, so the exchange area and the staging patches meet the next tile's prologue DMA.
# Transposed: the forward walks; conv: the input gradient walks
WALK_GEOMS = {
    "walk_T_64to64": Geom(4, 32, 32, 64, 64, 64, 64, 4, 4, 2, 2, 1, 1, True),
    "walk_C_64to64": Geom(4, 32, 32, 64, 64, 64, 64, 4, 4, 2, 2, 1, 1, False),
}
# the same walk WITHOUT a split (the plain epilogue, then the next tile's prologue DMA): more than the 512 resident blocks of a
# launch.  17 x 32 x 32 = 17408 rows per phase are 136 (tile 17) / 272 (tile 18) M tiles, four phases, one column tile ->
# 512 / 4 = 128 blocks per phase, so blocks walk two (tile 17: some of them) to three M tiles.  32 channels keep it small
WALK1_GEOMS = {
    "walk1_T_32to32": Geom(17, 32, 32, 64, 64, 32, 32, 4, 4, 2, 2, 1, 1, True),
    "walk1_C_32to32": Geom(17, 32, 32, 64, 64, 32, 32, 4, 4, 2, 2, 1, 1, False),
}


def _wide(shape, gen):
    t = torch.randn(shape, generator=gen) * torch.exp2(torch.randint(-12, 13, shape, generator=gen).float())
    t.view(-1)[: t.numel() // 7] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs on the device and the fp64 truths of one geometry: computed once, shared by the tests, never written to"""
    g = GEOMS.get(name) or WALK_GEOMS.get(name) or WALK1_GEOMS[name]
    gen = torch.Generator().manual_seed(29 + len(name))
    x, dy, wp = _wide(g.in_shape, gen), _wide(g.out_shape, gen), _wide((g.taps, g.Cin, g.Cout), gen)
    xd, wd, dyd = x.to(DEV), wp.to(DEV), dy.to(DEV)
    y64 = TB.conv_fwd(xd.double(), wd.double(), g)
    dx64 = TB.conv_dgrad(dyd.double(), wd.double(), g)
    return g, (x, wp, dy), (xd, wd, dyd), y64, dx64


def _assert_fp32_result(tag, got, native, ref64):
    l2e, l2n = _err64(got, ref64)[0], _err64(native, ref64)[0]
    _log(f"kpart/{tag}: relL2 vs fp64 {l2e:.3e}  (fp32-MFMA tile {l2n:.3e})")
    assert torch.isfinite(got).all(), tag
    assert l2e <= 1.05 * l2n, (tag, l2e, l2n)
    assert l2e < 2e-6, (tag, l2e)


@pytest.mark.parametrize("name", list(GEOMS))
def test_kpartition_against_fp64(name):
    """forward and input gradient of every small geometry, without a split and with uneven / empty split ranges"""
    g, _, (xd, wd, dyd), y64, dx64 = _case(name)
    for tile, native in KPART:
        for split in (1, 2, 3, 5):
            with ops.force_plan(native, split):
                yn, dxn = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
            with ops.force_plan(tile, split):
                y, dx = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
            _assert_fp32_result(f"{name}/t{tile}s{split}/fwd", y, yn, y64)
            _assert_fp32_result(f"{name}/t{tile}s{split}/dgrad", dx, dxn, dx64)


@pytest.mark.parametrize("name", list(WALK_GEOMS))
def test_kpartition_persistent_m_loop(name):
    """a block walks several M tiles: EVERY output element against fp64 (a race between the exchange and the next tile's
    operand DMA shows as a few wrong tiles), and the fp32-result criterion on the whole tensor"""
    g, _, (xd, wd, dyd), y64, dx64 = _case(name)
    for tile, native in KPART:
        with ops.force_plan(native, 8):
            yn, dxn = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
        with ops.force_plan(tile, 8):
            y, dx = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
        _assert_fp32_result(f"{name}/t{tile}s8/fwd", y, yn, y64)
        _assert_fp32_result(f"{name}/t{tile}s8/dgrad", dx, dxn, dx64)
        check(f"kpart/{name}/t{tile}s8/fwd_every_element", y, y64)
        check(f"kpart/{name}/t{tile}s8/dgrad_every_element", dx, dx64)


@pytest.mark.parametrize("name", list(WALK1_GEOMS))
def test_kpartition_persistent_m_loop_without_split(name):
    """the walk with plan split 1: every output element against fp64, the fp32-result criterion, and the same bits twice"""
    g, _, (xd, wd, dyd), y64, dx64 = _case(name)
    for tile, native in KPART:
        with ops.force_plan(native, 1):
            yn, dxn = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
        with ops.force_plan(tile, 1):
            y, dx = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
            y1, dx1 = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
        _assert_fp32_result(f"{name}/t{tile}s1/fwd", y, yn, y64)
        _assert_fp32_result(f"{name}/t{tile}s1/dgrad", dx, dxn, dx64)
        check(f"kpart/{name}/t{tile}s1/fwd_every_element", y, y64)
        check(f"kpart/{name}/t{tile}s1/dgrad_every_element", dx, dx64)
        assert torch.equal(y, y1) and torch.equal(dx, dx1), (name, tile)


@pytest.mark.parametrize("name", ["t_k4s2_96to32_odd", "c_k4s2_64to96"])
def test_kpartition_every_epilogue_feature(name):
    """forward with bias, channel mask, statistics and the residual mix; input gradient with ReLU/BN masking and bwd_sums"""
    g, (x, wp, dy), (xd, wd, dyd), _, _ = _case(name)
    gen = torch.Generator().manual_seed(13)
    rows_in, rows_out = x.numel() // g.Cin, math.prod(g.out_shape[:3])
    bias = 0.1 * torch.randn(g.Cout, generator=gen)
    bn = make_bn(g.Cin, rows_in, 1, gen, x)
    cmask = Mask((torch.rand(g.N, g.Cout, generator=gen) < 0.5).float() * 2, 1, rows_out // g.N)
    sres = torch.randn(g.out_shape, generator=gen)
    bns = make_bn(g.Cout, rows_out, 1, gen, sres)
    st_ref = torch.zeros(2, g.Cout, dtype=torch.float64)
    y_ref = TB.conv_fwd(x, wp, g, bias=bias, mask=cmask, out_stats=st_ref, mix=(sres, bns))
    ss_ref = torch.zeros(2, g.Cout, dtype=torch.float64)
    y_short = TB.conv_fwd(x, wp, g, bias=bias, mask=cmask, out_stats=ss_ref)
    s_ref = torch.zeros(2, g.Cin, dtype=torch.float64)
    dx_ref = TB.conv_dgrad(dy, wp, g, relu_bn=bn, xin=x, bwd_sums=s_ref)
    bd, bnd, cmd, mixd = bias.to(DEV), to_dev(bn), to_dev(cmask), (sres.to(DEV), to_dev(bns))
    for tile, _native in KPART:
        for split in (1, 3):
            tag = f"kpart/{name}/t{tile}s{split}"
            with ops.force_plan(tile, split):
                st = torch.zeros(2, g.Cout, dtype=torch.float64, device=DEV)
                check(f"{tag}/fwd_mix", ops.conv_fwd(xd, wd, g, bias=bd, mask=cmd, out_stats=st, mix=mixd), y_ref)
                check(f"{tag}/fwd_mix_stats", st, st_ref, rtol=1e-4, atol_rel=1e-4)
                st = torch.zeros(2, g.Cout, dtype=torch.float64, device=DEV)
                check(f"{tag}/fwd_stats_y", ops.conv_fwd(xd, wd, g, bias=bd, mask=cmd, out_stats=st), y_short)
                check(f"{tag}/fwd_stats", st, ss_ref, rtol=1e-4, atol_rel=1e-4)
                s = torch.zeros(2, g.Cin, dtype=torch.float64, device=DEV)
                check(f"{tag}/dgrad_relubn", ops.conv_dgrad(dyd, wd, g, relu_bn=bnd, xin=xd, bwd_sums=s), dx_ref)
                check(f"{tag}/dgrad_sums", s, s_ref, rtol=2e-4, atol_rel=2e-4)
                with pytest.raises(ops.MopoeHipError):      # the refusal rule stays: no BN-on-load form
                    ops.conv_fwd(xd, wd, g, bn_in=bnd)


@pytest.mark.parametrize("name", ["c1x1_32to96_r40", "t_k4s2_96to32_odd", "walk_T_64to64"])
def test_kpartition_deterministic_without_split(name):
    """no split reduction -> no atomics and no arrival order anywhere: two launches give the same bits"""
    g, _, (xd, wd, dyd), _, _ = _case(name)
    for tile, _native in KPART:
        with ops.force_plan(tile, 1):
            y0, dx0 = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
            y1, dx1 = ops.conv_fwd(xd, wd, g), ops.conv_dgrad(dyd, wd, g)
        assert torch.equal(y0, y1) and torch.equal(dx0, dx1), (name, tile)
