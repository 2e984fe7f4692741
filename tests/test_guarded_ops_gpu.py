"""Guard-band and hostile-value tests: every family of the C ABI (include/mopoe_hip.h) inside the arena of tests/arena.py.

The other per-kernel tests hand the kernels tight, fresh, 16-byte aligned tensors, zeroed accumulators and randn values.
Here every input and every result lives in a buffer of NaN poison with at least max(1 MiB, 256 rows) of guard on both
sides, and one harness (`guarded`) checks for each call that

  (a) no byte outside the placed tensors changed (an overrun of a row, a vector or a tile lands in a guard),
  (b) every result -- returned or merely allocated by mimic_amd.ops -- is finite (a read past an input that reaches a result
      brings NaN with it; a result left partly unwritten is still poison),
  (c) every input is bit-identical to its copy, except the accumulators / in-place operands the header documents,
  (d) the results meet the bars of the existing tests against the references of tests/torch_backend*.py, in fp32 and --
      wherever the reference takes doubles -- against its fp64 evaluation,

and that the head of the conv workspace (arrival counters) and the latent / likelihood workspaces are zero afterwards, the
conv workspace's scratch region having been filled with NaN before the launch.  Accumulators documented as "+=" start from
known non-zero values.  Nothing here is meant to fault: an overrun is observed in owned memory.

Entry point -> the test that calls it under the arena (tests/test_arena_cpu.py checks this table against the header):

    mopoe_conv_fwd                   -> test_conv_fp32
    mopoe_conv_fwd_mix               -> test_conv_fp32
    mopoe_conv_dgrad                 -> test_conv_fp32
    mopoe_conv_wgrad                 -> test_conv_fp32
    mopoe_block_out_fwd              -> test_glue_fp32
    mopoe_bn_relu_apply              -> test_glue_fp32
    mopoe_bn_bwd_reduce              -> test_glue_fp32
    mopoe_block_out_bwd              -> test_glue_fp32
    mopoe_bn_bwd_apply               -> test_glue_fp32
    mopoe_colsum                     -> test_glue_fp32
    mopoe_bn_running_update          -> test_bn_running_update
    mopoe_latent_fwd                 -> test_latent
    mopoe_latent_bwd                 -> test_latent
    mopoe_latent_mixture_fwd         -> test_latent_mixture
    mopoe_latent_mixture_bwd         -> test_latent_mixture
    mopoe_latent_style_fwd           -> test_latent_style
    mopoe_latent_style_bwd           -> test_latent_style
    mopoe_laplace_nll_fwd            -> test_likelihoods
    mopoe_laplace_nll_bwd            -> test_likelihoods
    mopoe_logsoftmax_fwd             -> test_likelihoods
    mopoe_logsoftmax_bwd             -> test_likelihoods
    mopoe_logsoftmax_bwd_bf16out     -> test_likelihoods
    mopoe_token_nll_fwd              -> test_likelihoods
    mopoe_token_nll_bwd              -> test_likelihoods
    mopoe_token_softmax_grad         -> test_likelihoods
    mopoe_dense_nll_fwd              -> test_likelihoods
    mopoe_dense_nll_bwd              -> test_likelihoods
    mopoe_lse_rows                   -> test_vocabulary_head
    mopoe_token_nll_logits_fwd       -> test_vocabulary_head
    mopoe_token_softmax_grad_logits  -> test_vocabulary_head
    mopoe_laplace_logprob_rows       -> test_logprob_rows
    mopoe_token_logprob_rows         -> test_logprob_rows
    mopoe_dense_logprob_rows         -> test_logprob_rows
    mopoe_lhood_style_sample         -> test_lhood_estimator
    mopoe_lhood_estimates            -> test_lhood_estimator
    mopoe_logreg_fit                 -> test_logreg
    mopoe_logreg_predict             -> test_logreg
    mopoe_embedding_fwd              -> test_embedding
    mopoe_embedding_bwd              -> test_embedding
    mopoe_embedding_fwd_bf16         -> test_embedding
    mopoe_embedding_bwd_bf16         -> test_embedding
    mopoe_block_front_stats          -> test_block_front
    mopoe_block_front_apply          -> test_block_front
    mopoe_block_front_bwd            -> test_block_front
    mopoe_block_front_stats_bf16     -> test_block_front
    mopoe_block_front_apply_bf16     -> test_block_front
    mopoe_block_front_bwd_bf16       -> test_block_front
    mopoe_conv_fwd_bf16              -> test_conv_bf16
    mopoe_conv_fwd_mix_bf16          -> test_conv_bf16
    mopoe_conv_dgrad_bf16            -> test_conv_bf16
    mopoe_conv_wgrad_bf16            -> test_conv_bf16
    mopoe_edge_expand_bf16           -> test_edge_layers_bf16
    mopoe_edge_wgrad_bf16            -> test_edge_layers_bf16
    mopoe_edge_reduce_bf16           -> test_edge_layers_bf16
    mopoe_bn_relu_apply_bf16         -> test_glue_bf16
    mopoe_block_out_fwd_bf16         -> test_glue_bf16
    mopoe_bn_bwd_reduce_bf16         -> test_glue_bf16
    mopoe_block_out_bwd_bf16         -> test_glue_bf16
    mopoe_bn_bwd_apply_bf16          -> test_glue_bf16
    mopoe_colsum_bf16                -> test_glue_bf16
    mopoe_adam_step                  -> test_adam_step

Exempt (they write no caller-owned device tensor): mopoe_abi_version and mopoe_last_error return host values;
mopoe_conv_workspace_bytes returns a size; mopoe_prof_enable / mopoe_prof_collect / mopoe_prof_stamp are the profiling hooks
of bench.py and of the timeline tool (host-side event bookkeeping; the stamp is a one-thread kernel storing 8 bytes into a slot
the tool owns, outside every training and evaluation path).

BatchNorm at shifted means (test_bn_shifted_means; the hostile input sets are pinned by tests/test_arena_cpu.py, where the
fp32 reference arithmetic has to stay within half of the bar on them): error against fp64 of the kernels and of
torch.nn.functional.batch_norm + autograd in fp32 on the CPU, gate kernel <= 4 x reference + the floor of `check` for a
shift r <= 30 (in units of the channel's spread), r = 100 logged.  The measured ratios are in DESIGN.md section 8.
"""
import math
import re

import numpy as np
import pytest
import torch

import torch_backend as TB
import torch_backend_lhood as TBL
import torch_backend_methods as TBM
import torch_backend_style as TBS
import torch_backend_lr as TBLR
import lr_util as LU
import hostile_sets as HS
from arena import Arena, ArenaError, outputs_in, CALLED_UNDER_ARENA, POISON16
from mimic_amd import ops
from mimic_amd.mmvae import kl_weights, mixture_row_starts
from mimic_amd.ops import Bn, Geom, Mask
from test_hip_ops_gpu import check, make_bn, _log, GEOMS, PLAN_GEOMS, GLDS_GEOMS32
from test_bf16_gpu import check16, GEOMS16, ULP

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
STATS = (1e-4, 1e-4)        # the statistics bars of tests/test_hip_ops_gpu.py
SUMS = (2e-4, 2e-4)
STATS16 = (2e-3, 2e-3)      # ... and of tests/test_bf16_gpu.py
BAR_SCALE = 1.0             # tests/test_arena_cpu.py runs the hostile-value cases on the CPU references at half of every bar


@pytest.fixture(scope="module")
def arena():
    a = Arena(DEV)
    yield a
    _log("guarded: entry points called under the arena: " + " ".join(sorted(set().union(*CALLED_BY_TEST.values()))))


CALLED_BY_TEST = {}         # test function -> the entry points the library was asked for inside outputs_in during its cases


@pytest.fixture(autouse=True)
def _attribute_entry_points(request):
    CALLED_UNDER_ARENA.clear()
    yield
    CALLED_BY_TEST.setdefault(request.node.originalname, set()).update(CALLED_UNDER_ARENA)


def coverage_table():
    """entry point -> test, as the docstring of this file states it"""
    return dict(re.findall(r"^\s+(mopoe_[a-z0-9_]+)\s+->\s+(test_[a-z0-9_]+)\s*$", __doc__, flags=re.M))


# ---- the harness ---------------------------------------------------------------------------------------------------------
def _map(obj, fn, path=""):
    if isinstance(obj, torch.Tensor):
        return fn(path, obj)
    if isinstance(obj, Bn):
        f = lambda k: _map(getattr(obj, k), fn, f"{path}.{k}")
        return Bn(f("gamma"), f("beta"), obj.mode, f("sums"), obj.count, f("rmean"), f("rvar"), obj.eps)
    if isinstance(obj, Mask):
        return Mask(_map(obj.mask, fn, f"{path}.mask"), obj.kind, obj.rows_per_sample)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map(v, fn, f"{path}[{i}]") for i, v in enumerate(obj))
    if isinstance(obj, dict):
        return {k: _map(v, fn, f"{path}.{k}" if path else k) for k, v in obj.items()}
    return obj


def _leaves(obj):
    out = []
    _map(obj, lambda p, t: out.append((p, t)) or t)
    return out


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _to64(obj):
    """the same inputs with the fp32 tensors of the TOP level as doubles (BatchNorm / mask records stay as they are: the
    references form the coefficients in fp32 like the kernels do)"""
    return {k: (v.double() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else
                [None if t is None else (t.double() if t.dtype == torch.float32 else t) for t in v]
                if isinstance(v, list) and all(t is None or isinstance(t, torch.Tensor) for t in v) else v)
            for k, v in obj.items()}


def _is_under(path, roots):
    return any(path == r or path.startswith(r + ".") or path.startswith(r + "[") for r in roots)


def _compare(name, got, ref, bar):
    if callable(bar):
        return bar(name, got, ref)
    if bar == "eq":
        assert torch.equal(got.cpu(), ref.to(got.dtype)), name
        return
    if got.dtype == BF:
        check16(name, got, ref.to(BF), **({} if bar is None else {"atol_rel": bar[1]}))
    else:
        rtol, atol_rel = (2e-4, 2e-4) if bar is None else bar        # (None: the defaults of check)
        check(name, got, ref, rtol=BAR_SCALE * rtol, atol_rel=BAR_SCALE * atol_rel)


def _conv_ws():
    return ops._workspace(torch.device(DEV, 0) if DEV == "cuda" else torch.device(DEV))


def _dirty_workspaces():
    """conv workspace: scratch beyond the 64 KiB of arrival counters filled with NaN (a launch writes it before it reads
    it); every workspace is created here, outside the arena"""
    ws, n = _conv_ws()
    ws[ops.WS_COUNTER_BYTES:ops.WS_COUNTER_BYTES + (n - ops.WS_COUNTER_BYTES) // 2 * 2].view(torch.int16).fill_(POISON16)
    for k in (8, 16, 4):
        ops._ws(ws.device, k)


def _check_workspaces(tag):
    ws, _n = _conv_ws()
    assert not bool(ws[:ops.WS_COUNTER_BYTES].any()), f"{tag}: arrival counters of the conv workspace left non-zero"
    for key, t in ops._kl_ws.items():
        assert not bool(t.any()), f"{tag}: latent / likelihood workspace {key} left non-zero"


def guarded(arena, tag, inputs, call, ref, bars=None, inout=(), misalign=None, ref64=True, raises=False):
    """inputs: dict name -> CPU tensor / Bn / Mask / list of tensors / plain value.  call(placed) runs the op on the placed
    (device) objects and returns a dict name -> result tensor (None entries are skipped); ref: callable(inputs) -> dict of
    references, or such a dict (or a list of them) computed beforehand; bars: name -> None (the default bars of check /
    check16), (rtol, atol_rel), "eq" or a callable(name, got, ref); inout: names of inputs the op may write (accumulators,
    in-place operands); misalign: path -> bytes off a 16-byte boundary; raises: the call has to be refused with
    MopoeHipError before anything is launched (every result of the arena still pure poison)."""
    arena.reset()
    bars, misalign = bars or {}, misalign or {}
    placed = _map(inputs, lambda p, t: arena.place(t, misalign.get(p, 0), name=p))
    assert set(misalign) <= {p for p, _ in _leaves(placed)}, (tag, misalign)
    clones = _map(placed, lambda p, t: t.clone())
    _dirty_workspaces()
    with outputs_in(arena) as px:
        if raises:
            with pytest.raises(ops.MopoeHipError):
                call(placed)
            got = {}
        else:
            got = call(placed)
    if DEV == "cuda":
        torch.cuda.synchronize()
    arena.assert_untouched()                                                            # (a)
    if raises:
        for t in px.allocated:     # (zero-filled requests -- the accumulators ops.py creates -- are still all zero)
            clean = not bool(t.any()) if t.data_ptr() in px.zero_filled else arena.is_poison(t)
            assert clean, f"{tag}: a refused call wrote a result"
        for (p, t), (_, c) in zip(_leaves(placed), _leaves(clones)):
            assert torch.equal(_bits(t), _bits(c)), f"{tag}: a refused call modified {p}"
        _check_workspaces(tag)
        return None
    for i, t in enumerate(px.allocated):                                                # (b)
        assert bool(torch.isfinite(t.float()).all()), f"{tag}: result #{i} {tuple(t.shape)} allocated by ops is not finite"
    for name, t in got.items():
        if t is not None:
            assert bool(torch.isfinite(t.double()).all()), f"{tag}/{name}: not finite"
            if DEV == "cuda":
                assert arena.owns(t), f"{tag}/{name}: the result was not allocated in the arena"
    for (p, t), (_, c) in zip(_leaves(placed), _leaves(clones)):                        # (c)
        if not _is_under(p, inout):
            assert torch.equal(_bits(t), _bits(c)), f"{tag}: input {p} was modified"
    _check_workspaces(tag)
    if callable(ref):                                                                   # (d)
        refs = [ref(_map(inputs, lambda p, t: t.clone()))]
        if ref64:
            refs.append(ref(_to64(_map(inputs, lambda p, t: t.clone()))))
    else:
        refs = ref if isinstance(ref, list) else [ref]
    for k, r in enumerate(refs):
        for name, want in r.items():
            if want is not None:
                _compare(f"guarded/{tag}/{name}" + ("/fp64" if k else ""), got[name], want, bars.get(name))
    return got


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _prefill(shape, gen, dtype=torch.float64, scale=5.0):
    """known non-zero start of an accumulator the header documents as '+='"""
    return (scale * torch.randn(shape, generator=gen)).to(dtype) + 1.0


def _geom(name):
    for n, g in GEOMS + PLAN_GEOMS + GLDS_GEOMS32 + [("narrow_many_rows_C", Geom(16, 32, 32, 64, 64, 16, 8, 4, 4, 2, 2, 1, 1, False))]:
        if n == name:
            return g
    raise KeyError(name)


def _cmask(g, gen):
    return Mask((torch.rand(g.N, g.Cout, generator=gen) < 0.5).float() * 2, 1, math.prod(g.out_shape[1:3]))


# ---- detection itself: a plain torch write into a guard is reported --------------------------------------------------------
def test_a_guard_byte_written_with_torch_is_reported(arena):
    arena.reset()
    v = arena.place(torch.randn(37, 20), name="x")
    arena.assert_untouched()
    flat = arena.raw["h"]
    off = v.data_ptr() - flat.data_ptr()
    flat[off + v.numel() * 4 + 80] = 1                      # one byte, 80 bytes past the end: row 37 of a [*, 20] fp32 matrix
    with pytest.raises(ArenaError, match="80 bytes past the end of view 'x'"):
        arena.assert_untouched()
    arena.reset()
    arena.assert_untouched()


# ---- fp32 convolution family -----------------------------------------------------------------------------------------------
def _conv32_inputs(g, seed, bn_mode=1):
    gen = _gen(seed)
    x = torch.randn(g.in_shape, generator=gen)
    wp = torch.randn(g.taps, g.Cin, g.Cout, generator=gen) / math.sqrt(g.taps * g.Cin)
    bias = 0.1 * torch.randn(g.Cout, generator=gen)
    dy = torch.randn(g.out_shape, generator=gen)
    rows_in, rows_out = x.numel() // g.Cin, math.prod(g.out_shape[:3])
    bn = make_bn(g.Cin, rows_in, bn_mode, gen, x if bn_mode == 1 else None)
    sres = torch.randn(g.out_shape, generator=gen)
    bns = make_bn(g.Cout, rows_out, 1, gen, sres)
    return dict(x=x, wp=wp, bias=bias, dy=dy, bn=bn, mask=_cmask(g, gen), sres=sres, bns=bns,
                stats=_prefill((2, g.Cout), gen), sums=_prefill((2, g.Cin), gen))


def _pick(d, *names):
    return {k: d[k] for k in names}


def _fwd_call(g, bn=True, mix=False):
    def call(p):
        y = ops.conv_fwd(p["x"], p["wp"], g, bn_in=p["bn"] if bn else None, bias=p["bias"], mask=p["mask"], out_stats=p["stats"],
                         mix=(p["sres"], p["bns"]) if mix else None)
        return dict(y=y, stats=p["stats"])
    return call


def _fwd_ref(g, bn=True, mix=False):
    def ref(h):
        st = h["stats"].clone()
        y = TB.conv_fwd(h["x"], h["wp"], g, bn_in=h["bn"] if bn else None, bias=h["bias"], mask=h["mask"], out_stats=st,
                        mix=(h["sres"], h["bns"]) if mix else None)
        return dict(y=y, stats=st)
    return ref


def _dgrad_call(g, relu=True):
    def call(p):
        dx = ops.conv_dgrad(p["dy"], p["wp"], g, relu_bn=p["bn"] if relu else None, xin=p["x"] if relu else None,
                            bwd_sums=p["sums"] if relu else None)
        return dict(dx=dx, sums=p["sums"] if relu else None)
    return call


def _dgrad_ref(g, relu=True):
    def ref(h):
        s = h["sums"].clone()
        dx = TB.conv_dgrad(h["dy"], h["wp"], g, relu_bn=h["bn"] if relu else None, xin=h["x"] if relu else None,
                           bwd_sums=s if relu else None)
        return dict(dx=dx, sums=s if relu else None)
    return ref


def _wgrad_call(g, bn=False):
    return lambda p: dict(dw=ops.conv_wgrad(p["x"], p["dy"], g, bn_in=p["bn"] if bn else None))


def _wgrad_ref(g, bn=False):
    return lambda h: dict(dw=TB.conv_wgrad(h["x"], h["dy"], g, bn_in=h["bn"] if bn else None))


CONV32 = ["ragged_c20", "odd_grid_T_96to32", "stem_k3s2_cin1_ragged_rows", "dec_head_k3s2p1op1_ragged_rows", "linear_320to128",
          "text_vocab_k1", "narrow_many_rows_C"]


@pytest.mark.parametrize("name", CONV32)
def test_conv_fp32(arena, name):
    """forward with BN on load + bias + channel mask + statistics (accumulated onto a non-zero start), the residual mix where
    the vector path takes it, input gradient with relu_bn + sums (likewise accumulated), weight gradient plain, with a
    train-mode and -- new -- with an eval-mode (mode 2) BatchNorm on its operand"""
    g = _geom(name)
    h = _conv32_inputs(g, 100 + len(name))
    fwd_in = _pick(h, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns")
    guarded(arena, f"{name}/fwd", fwd_in, _fwd_call(g), _fwd_ref(g), bars=dict(stats=STATS), inout=("stats",))
    if ops.conv_mix_supported(h["x"], g):
        guarded(arena, f"{name}/fwd_mix", fwd_in, _fwd_call(g, mix=True), _fwd_ref(g, mix=True), bars=dict(stats=STATS), inout=("stats",))
    dg_in = _pick(h, "x", "wp", "dy", "bn", "sums")
    guarded(arena, f"{name}/dgrad", dg_in, _dgrad_call(g), _dgrad_ref(g), bars=dict(sums=SUMS), inout=("sums",))
    guarded(arena, f"{name}/dgrad_plain", dg_in, _dgrad_call(g, False), _dgrad_ref(g, False))
    wg_in = _pick(h, "x", "dy", "bn")
    guarded(arena, f"{name}/wgrad", wg_in, _wgrad_call(g), _wgrad_ref(g))
    guarded(arena, f"{name}/wgrad_bn1", wg_in, _wgrad_call(g, True), _wgrad_ref(g, True))
    # out=: the caller's zero-filled slice (dwp_is_zero: the library skips its memset; the header documents no "+=" here)
    guarded(arena, f"{name}/wgrad_out", dict(wg_in, out=torch.zeros(g.taps, g.Cin, g.Cout)),
            lambda p: dict(dw=ops.conv_wgrad(p["x"], p["dy"], g, out=p["out"])), _wgrad_ref(g), inout=("out",))
    if name in ("ragged_c20", "odd_grid_T_96to32"):
        h2 = _conv32_inputs(g, 200 + len(name), bn_mode=2)
        guarded(arena, f"{name}/wgrad_bn2", _pick(h2, "x", "dy", "bn"), _wgrad_call(g, True), _wgrad_ref(g, True))
        guarded(arena, f"{name}/fwd_bn2", _pick(h2, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns"), _fwd_call(g), _fwd_ref(g),
                bars=dict(stats=STATS), inout=("stats",))


WIDE_WGRAD_GEOMS = ("linear_320to128", "enc_1x1_128")     # more than 64 channels on both sides: the 128 x 128 LDS-DMA tiles
FWD_TILES = (0, 1, 2, 3, 4, 8, 12, 13, 14, 15, 16, 17, 18, 19)
BN_ON_LOAD_TILES = (0, 1, 2, 3, 4, 8, 12, 14, 15)


def test_conv_fp32_forced_plans(arena):
    """enc_64to128_b9_ragged (576 output rows: several row tiles and a partial last one) on every tile the header lists that
    accepts it, unsplit and with the reduction split three ways: the split launches park partial sums in the (NaN-filled)
    workspace and must leave the arrival counters zero.  The weight-gradient tiles 5 and 7 (128 x 128 on LDS-DMA) refuse its
    64 input channels -- checked as a refusal -- and are launched on WIDE_WGRAD_GEOMS instead"""
    g = _geom("enc_64to128_b9_ragged")
    h = _conv32_inputs(g, 77)
    fwd_in = _pick(h, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns")
    dg_in = _pick(h, "x", "wp", "dy", "bn", "sums")
    wg_in = _pick(h, "x", "dy", "bn")
    refs = {(bn, mix): [_fwd_ref(g, bn, mix)(fwd_in), _fwd_ref(g, bn, mix)(_to64(fwd_in))] for bn in (True, False) for mix in (True, False)}
    dref = [_dgrad_ref(g)(dg_in), _dgrad_ref(g)(_to64(dg_in))]
    wref = [_wgrad_ref(g)(wg_in), _wgrad_ref(g)(_to64(wg_in))]
    for tile in FWD_TILES:
        for split in (1, 3):
            bn = tile in BN_ON_LOAD_TILES
            with ops.force_plan(tile, split):
                for mix in (False, True):
                    guarded(arena, f"plan/t{tile}s{split}/fwd{'_mix' if mix else ''}", fwd_in, _fwd_call(g, bn, mix), refs[(bn, mix)],
                            bars=dict(stats=STATS), inout=("stats",))
                guarded(arena, f"plan/t{tile}s{split}/dgrad", dg_in, _dgrad_call(g), dref, bars=dict(sums=SUMS), inout=("sums",))
    for tile in (0, 2, 5, 6, 7, 8, 9, 10):
        for split in (1, 3):
            with ops.force_plan(tile, split):
                # (the 128 x 128 LDS-DMA tiles need more than 64 channels on both sides: refused, nothing launched)
                guarded(arena, f"plan/wgrad_t{tile}s{split}", wg_in, _wgrad_call(g), wref, bars=dict(dw=(5e-4, 5e-4)),
                        raises=tile in (5, 7))
    # ... which therefore run where they are accepted: linear_320to128 (2.5 row tiles of channels, 7 pixels: one partial
    # stage, a split clamps to 1) and enc_1x1_128 (512 pixels: the split of three is real); 7 has no BN-on-load form
    for name in WIDE_WGRAD_GEOMS:
        gw = _geom(name)
        hw = _conv32_inputs(gw, 79 + len(name))
        ww_in = _pick(hw, "x", "dy", "bn")
        for bn in (False, True):
            ref = [_wgrad_ref(gw, bn)(ww_in), _wgrad_ref(gw, bn)(_to64(ww_in))]
            for tile in (5, 7):
                for split in (1, 3):
                    with ops.force_plan(tile, split):
                        guarded(arena, f"plan/{name}/wgrad{'_bn' if bn else ''}_t{tile}s{split}", ww_in, _wgrad_call(gw, bn), ref,
                                bars=dict(dw=(5e-4, 5e-4)), raises=bn and tile == 7)


# ---- bf16 convolution family -----------------------------------------------------------------------------------------------
def _conv16_inputs(g, seed):
    gen = _gen(seed)
    x = torch.randn(g.in_shape, generator=gen).to(BF)
    wp = (torch.randn(g.taps, g.Cin, g.Cout, generator=gen) / math.sqrt(g.taps * g.Cin)).to(BF)
    bias = 0.1 * torch.randn(g.Cout, generator=gen)
    dy = torch.randn(g.out_shape, generator=gen).to(BF)
    rows_in, rows_out = x.numel() // g.Cin, math.prod(g.out_shape[:3])
    bn = make_bn(g.Cin, rows_in, 1, gen, x.float())
    sres = torch.randn(g.out_shape, generator=gen).to(BF)
    bns = make_bn(g.Cout, rows_out, 1, gen, sres.float())
    return dict(x=x, wp=wp, bias=bias, dy=dy, bn=bn, mask=_cmask(g, gen), sres=sres, bns=bns,
                stats=_prefill((2, g.Cout), gen), sums=_prefill((2, g.Cin), gen))


def _fwd16(g, bn, mix, f32=False):
    kw = dict(out_dtype=torch.float32) if f32 else {}

    def call(p):
        y = ops.conv_fwd(p["x"], p["wp"], g, bn_in=p["bn"] if bn else None, bias=p["bias"], mask=p["mask"], out_stats=p["stats"],
                         mix=(p["sres"], p["bns"]) if mix else None, **kw)
        return dict(y=y, stats=p["stats"])

    def ref(h):
        st = h["stats"].clone()
        y = TB.conv_fwd(h["x"], h["wp"], g, bn_in=h["bn"] if bn else None, bias=h["bias"], mask=h["mask"], out_stats=st,
                        mix=(h["sres"], h["bns"]) if mix else None, **kw)
        return dict(y=y, stats=st)
    return call, ref


def _dgrad16(g, relu, f32=False):
    kw = dict(out_dtype=torch.float32) if f32 else {}

    def call(p):
        dx = ops.conv_dgrad(p["dy"], p["wp"], g, relu_bn=p["bn"] if relu else None, xin=p["x"] if relu else None,
                            bwd_sums=p["sums"] if relu else None, **kw)
        return dict(dx=dx, sums=p["sums"] if relu else None)

    def ref(h):
        s = h["sums"].clone()
        dx = TB.conv_dgrad(h["dy"], h["wp"], g, relu_bn=h["bn"] if relu else None, xin=h["x"] if relu else None,
                           bwd_sums=s if relu else None, **kw)
        return dict(dx=dx, sums=s if relu else None)
    return call, ref


RAGGED16 = ["odd_grid_k4s2p1_b3", "odd_grid_T_k4s2p1", "enc_k4s2p0_4to1", "linear_320to128", "text_conv1d_to1"]
Y16_BN = dict(y=(0, 1.5e-3), stats=STATS16)      # (the wider absolute term of test_bf16_gpu._conv_case for BN'd operands)


def _conv16_case(arena, tag, g, h, wgrad_bn=True):
    fwd_in = _pick(h, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns")
    dg_in = _pick(h, "x", "wp", "dy", "bn", "sums")
    c, r = _fwd16(g, True, False)
    guarded(arena, f"{tag}/fwd", fwd_in, c, r, bars=Y16_BN, inout=("stats",), ref64=False)
    c, r = _fwd16(g, False, False, f32=True)
    guarded(arena, f"{tag}/fwd_f32out", fwd_in, c, r, bars=dict(stats=STATS16), inout=("stats",), ref64=False)
    c, r = _fwd16(g, True, True)
    guarded(arena, f"{tag}/fwd_mix", fwd_in, c, r, bars=Y16_BN, inout=("stats",), ref64=False)
    c, r = _dgrad16(g, True)
    guarded(arena, f"{tag}/dgrad", dg_in, c, r, bars=dict(sums=STATS16), inout=("sums",), ref64=False)
    c, r = _dgrad16(g, False, f32=True)
    guarded(arena, f"{tag}/dgrad_f32out", dg_in, c, r, ref64=False)
    wg_in = _pick(h, "x", "dy", "bn")
    guarded(arena, f"{tag}/wgrad", wg_in, _wgrad_call(g), _wgrad_ref(g), bars=dict(dw=(3e-4, 3e-4)), ref64=False)
    if wgrad_bn:
        guarded(arena, f"{tag}/wgrad_bn", wg_in, _wgrad_call(g, True), _wgrad_ref(g, True), bars=dict(dw=(2e-3, 1e-3)), ref64=False)


@pytest.mark.parametrize("name", RAGGED16)
def test_conv_bf16(arena, name):
    """the ragged members of GEOMS16 on the library's own plan: forward (BN on load + bias + mask + accumulated statistics;
    fp32 result; residual mix), input gradient (relu_bn + accumulated sums; fp32 result), weight gradient"""
    g = dict(GEOMS16)[name]
    _conv16_case(arena, name, g, _conv16_inputs(g, 300 + len(name)))


def test_conv_bf16_forced_plans(arena):
    """enc_k4s2p1_64to128_b9_ragged on tiles 0-7 and 9-11 (8 is refused), weight-gradient tiles 0, 2, 5-9, each unsplit and
    split three ways; weight-gradient tile 5 refuses 64 input channels and is launched on WIDE_WGRAD_GEOMS"""
    g = Geom(9, 8, 8, 16, 16, 64, 128, 4, 4, 2, 2, 1, 1, False)
    h = _conv16_inputs(g, 78)
    fwd_in = _pick(h, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns")
    dg_in = _pick(h, "x", "wp", "dy", "bn", "sums")
    wg_in = _pick(h, "x", "dy", "bn")
    fref = {bn: _fwd16(g, bn, False)[1](fwd_in) for bn in (True, False)}
    dref = _dgrad16(g, True)[1](dg_in)
    wref = _wgrad_ref(g)(wg_in)
    for tile in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        for split in (1, 3):
            bn = tile in (0, 1, 2, 3, 4, 5, 7, 9, 11)
            with ops.force_plan(tile, split):
                guarded(arena, f"plan16/t{tile}s{split}/fwd", fwd_in, _fwd16(g, bn, False)[0], fref[bn],
                        bars=Y16_BN if bn else dict(stats=STATS16), inout=("stats",), raises=tile == 8)
                guarded(arena, f"plan16/t{tile}s{split}/dgrad", dg_in, _dgrad16(g, True)[0], dref, bars=dict(sums=STATS16),
                        inout=("sums",), raises=tile == 8)
    for tile in (0, 2, 5, 6, 7, 8, 9):
        for split in (1, 3):
            with ops.force_plan(tile, split):
                guarded(arena, f"plan16/wgrad_t{tile}s{split}", wg_in, _wgrad_call(g), wref, bars=dict(dw=(3e-4, 3e-4)), raises=tile == 5)
    # tile 5 (refused above: 64 channels on one side) where it is accepted, plain and with BN on load
    for name in WIDE_WGRAD_GEOMS:
        gw = dict(GEOMS16)[name]
        hw = _conv16_inputs(gw, 80 + len(name))
        ww_in = _pick(hw, "x", "dy", "bn")
        for bn, bar in ((False, (3e-4, 3e-4)), (True, (2e-3, 1e-3))):
            ref = _wgrad_ref(gw, bn)(ww_in)
            for split in (1, 3):
                with ops.force_plan(5, split):
                    guarded(arena, f"plan16/{name}/wgrad{'_bn' if bn else ''}_t5s{split}", ww_in, _wgrad_call(gw, bn), ref, bars=dict(dw=bar))


@pytest.mark.parametrize("n,hs,ws", [(2, 16, 16), (3, 5, 16), (2, 6, 6)])
def test_edge_layers_bf16(arena, n, hs, ws):
    """image stem / head of the bf16 family (fp32 pixels and taps, bf16 wide tensor): the three shapes of
    test_bf16_gpu.test_edge_layers_bf16 (MFMA form, partial tile, streaming kernels)"""
    gen = _gen(5)
    gs = Geom(n, hs, ws, 2 * hs, 2 * ws, 1, 64, 3, 3, 2, 2, 1, 1, False)
    gh = Geom(n, hs, ws, 2 * hs, 2 * ws, 64, 1, 3, 3, 2, 2, 1, 1, True)
    h = dict(img=torch.rand(gs.in_shape, generator=gen), w=torch.randn(9, 1, 64, generator=gen) / 3, stats=_prefill((2, 64), gen),
             dy=torch.randn(gs.out_shape, generator=gen).to(BF), x=torch.randn(gh.in_shape, generator=gen).to(BF),
             wh=torch.randn(9, 64, 1, generator=gen) / 8, b=torch.tensor([0.3]), gimg=torch.randn(gh.out_shape, generator=gen))

    def stem(f):
        def run(p):
            st = p["stats"] if f is ops else p["stats"].clone()
            return dict(y=f.conv_fwd(p["img"], p["w"], gs, out_stats=st, out_dtype=BF), stats=st)
        return run
    guarded(arena, "edge/stem_fwd", _pick(h, "img", "w", "stats"), stem(ops), stem(TB), bars=dict(stats=STATS16), inout=("stats",), ref64=False)
    guarded(arena, "edge/stem_wgrad", _pick(h, "img", "dy"), lambda p: dict(dw=ops.conv_wgrad(p["img"], p["dy"], gs)),
            lambda p: dict(dw=TB.conv_wgrad(p["img"], p["dy"], gs)), bars=dict(dw=(3e-4, 3e-4)), ref64=False)
    guarded(arena, "edge/head_fwd", _pick(h, "x", "wh", "b"), lambda p: dict(y=ops.conv_fwd(p["x"], p["wh"], gh, bias=p["b"])),
            lambda p: dict(y=TB.conv_fwd(p["x"], p["wh"], gh, bias=p["b"])), ref64=False)
    guarded(arena, "edge/head_dgrad", _pick(h, "gimg", "wh"), lambda p: dict(dx=ops.conv_dgrad(p["gimg"], p["wh"], gh, out_dtype=BF)),
            lambda p: dict(dx=TB.conv_dgrad(p["gimg"], p["wh"], gh, out_dtype=BF)), ref64=False)
    guarded(arena, "edge/head_wgrad", _pick(h, "x", "gimg"), lambda p: dict(dw=ops.conv_wgrad(p["x"], p["gimg"], gh)),
            lambda p: dict(dw=TB.conv_wgrad(p["x"], p["gimg"], gh)), bars=dict(dw=(3e-4, 3e-4)), ref64=False)


# ---- the front of a residual block -------------------------------------------------------------------------------------------
def _front_inputs(dtype, n=5, rps=32, seed=9):
    c, rows = 64, n * rps
    gen = _gen(seed)
    x = torch.randn(rows, c, generator=gen).to(dtype).view(n, rps, 1, c)
    w1 = (torch.randn(1, c, c, generator=gen) / 8).to(dtype)
    bias = 0.1 * torch.randn(c, generator=gen)
    bn1 = make_bn(c, rows, 1, gen, x.float())
    mask = Mask((torch.rand(n, c, generator=gen) < 0.5).float() * 2, 1, rps)
    st = torch.zeros(2, c, dtype=torch.float64)
    TB.block_front_stats(x, w1, bias, bn1, mask, st)
    bn2 = Bn(torch.rand(c, generator=gen) + 0.5, 0.1 * torch.randn(c, generator=gen), 1, st.clone(), rows)
    a2 = TB.block_front_apply(x, w1, bias, bn1, bn2, mask)
    dh2 = (torch.randn(rows, c, generator=gen).view(x.shape) * (a2.float() > 0)).to(dtype)
    mean2, rstd2, _, _ = TB.bn_coef(bn2)
    d1 = TB._front_d1(x, w1, bias, bn1, mask)[1]
    sums2 = torch.stack([dh2.float().reshape(rows, c).double().sum(0), (dh2.float() * ((d1 - mean2) * rstd2)).reshape(rows, c).double().sum(0)])
    return dict(x=x, w1=w1, bias=bias, bn1=bn1, bn2=bn2, mask=mask, dh2=dh2, sums2=sums2, stats=_prefill((2, c), gen),
                sums1=_prefill((2, c), gen), dw1=_prefill((1, c, c), gen, torch.float32, 0.5), dbias=_prefill((c,), gen, torch.float32, 0.5),
                dg=torch.full((c,), math.nan), dbt=torch.full((c,), math.nan))     # (assigned, not accumulated: they start from NaN)


def _front_runs(f):
    own = f is ops

    def stats(p):
        st = p["stats"] if own else p["stats"].clone()
        f.block_front_stats(p["x"], p["w1"], p["bias"], p["bn1"], p["mask"], st)
        return dict(stats=st)

    def apply(p):
        return dict(a2=f.block_front_apply(p["x"], p["w1"], p["bias"], p["bn1"], p["bn2"], p["mask"]))

    def bwd(p):
        acc = {k: (p[k] if own else p[k].clone()) for k in ("sums1", "dw1", "dbias", "dg", "dbt")}
        dh1 = f.block_front_bwd(p["x"], p["dh2"], p["w1"], p["bias"], p["bn1"], p["bn2"], p["mask"], p["sums2"], acc["sums1"], acc["dw1"],
                                acc["dbias"], acc["dg"], acc["dbt"])
        return dict(dh1=dh1, **acc)
    return stats, apply, bwd


@pytest.mark.parametrize("family", ["fp32", "bf16"])
def test_block_front(arena, family):
    """csrc/pointwise.hip at n = 5, rows_per_sample = 32 (five 32-row tiles: fewer than one block's eight waves), with
    stats_d1 / sums1 / dw1 / dbias accumulated onto non-zero starts"""
    f16 = family == "bf16"
    h = _front_inputs(BF if f16 else torch.float32)
    (s_o, a_o, b_o), (s_r, a_r, b_r) = _front_runs(ops), _front_runs(TB)
    rows = 160
    guarded(arena, f"front/{family}/stats", _pick(h, "x", "w1", "bias", "bn1", "mask", "stats"), s_o, s_r,
            bars=dict(stats=STATS16 if f16 else STATS), inout=("stats",), ref64=False)
    a2bar = (lambda n, a, b: check(n, a.float(), b.float(), rtol=2.5 * ULP, atol_rel=2e-3)) if f16 else None
    guarded(arena, f"front/{family}/apply", _pick(h, "x", "w1", "bias", "bn1", "bn2", "mask"), a_o, a_r, bars=dict(a2=a2bar), ref64=False)
    rstd2 = TB.bn_coef(h["bn2"])[1]
    if f16:
        noise = ULP * float(h["dh2"].float().abs().max()) * float((h["bn2"].gamma * rstd2).abs().max()) * rows ** 0.5 * 2
        bars = dict(dh1=lambda n, a, b: check(n, a.float(), b.float(), rtol=2.5 * ULP, atol_rel=4e-3), sums1=(5e-3, 5e-3), dw1=(2e-3, 2e-3))
    else:
        noise = 2.0 ** -22 * float(h["dh2"].abs().max()) * float((h["bn2"].gamma * rstd2).abs().max()) * rows ** 0.5 * 8 + 1e-5
        bars = dict(sums1=(5e-4, 5e-4), dw1=(5e-4, 5e-4))

    def dbias_bar(n, a, b):     # (the column sums of a BatchNorm backward are analytically zero: the bar of the existing tests)
        assert (a.cpu() - b).abs().max().item() <= noise, (n, (a.cpu() - b).abs().max().item(), noise)
    bars.update(dbias=dbias_bar, dg=(1e-6, 1e-6), dbt=(1e-6, 1e-6))
    guarded(arena, f"front/{family}/bwd", h, b_o, b_r, bars=bars, inout=("sums1", "dw1", "dbias", "dg", "dbt", "stats"), ref64=False)


# ---- residual-block glue -------------------------------------------------------------------------------------------------------
def _glue_inputs(rows, c, dtype, seed, n=None):
    gen = _gen(seed)
    # (samples for the per-sample masks: four where the rows divide, else one row per sample -- the row count asked for is kept)
    n = n or (1 if rows < 8 else 4 if rows % 4 == 0 else rows)
    rps = rows // n
    assert n * rps == rows, (rows, n)
    mk = lambda: torch.randn(rows, c, generator=gen).to(dtype)
    s, m, g, x, add = mk(), mk(), mk(), mk(), mk()
    bn = make_bn(c, rows, 1, gen, s.float())
    bn2 = make_bn(c, rows, 2, gen)
    bnx = make_bn(c, rows, 1, gen, x.float())
    mean, rstd = TB.bn_coef(bnx)[:2]
    sums_x = torch.stack([g.float().double().sum(0), (g.float() * ((x.float() - mean) * rstd)).double().sum(0)])
    masks = [None, Mask((torch.rand(n, c, generator=gen) < 0.5).float() * 2, 1, rps),
             Mask((torch.rand(rows, c, generator=gen) < 0.5).float() * 2, 2, rps)]
    return dict(s=s, m=m, g=g, x=x, add=add, bn=bn, bn2=bn2, bnx=bnx, sums_x=sums_x, sums_s=TB.bn_bwd_reduce(g, s, bn), masks=masks,
                stats=_prefill((2, c), gen), rsum=_prefill((2, c), gen), nsum=_prefill((2, c), gen),
                # (dgamma / dbeta are ASSIGNED, the column sums accumulated: the first start from NaN, the others from known values)
                small4=torch.cat([torch.full((2, c), math.nan), _prefill((2, c), gen, torch.float32)]),
                small3=torch.cat([torch.full((2, c), math.nan), _prefill((1, c), gen, torch.float32)])), rows


def _colsum_zero_bar(scale_of, prefill, f16, rows):
    """column sums that are analytically ~0 (a train-mode BatchNorm backward): the bars of the existing tests, taken on what
    was ADDED to the pre-filled accumulator"""
    def bar(name, got, ref):
        err = ((got.double().cpu() - prefill.double()) - (ref.double() - prefill.double())).abs().max().item()
        bound = ULP * scale_of().float().abs().max().item() * rows ** 0.5 if f16 else 2e-5 * scale_of().abs().sum(0).max().item() + 1e-6
        bound += 4 * 2.0 ** -24 * float(prefill.abs().max())        # (fp32 rounding of the sum onto the pre-filled value)
        _log(f"{name}: err={err:.3e} bound={bound:.3e}")
        assert err <= bound, (name, err, bound)
    return bar


def _glue_case(arena, rows, c, dtype, seed, n=None):
    f16 = dtype == BF
    h, rows = _glue_inputs(rows, c, dtype, seed, n)
    tag = f"glue{'16' if f16 else ''}[{rows}x{c}]"
    st, sm = (STATS16 if f16 else STATS), (STATS16 if f16 else SUMS)
    r64 = not f16

    def runs(f):
        own = f is ops
        acc = lambda t: t if own else t.clone()

        def out_fwd(p):
            stt = acc(p["stats"])
            return dict(out=f.block_out_fwd(p["s"], p["m"], p["bn"], out_stats=stt), stats=stt)

        def reduce(p):
            if own:
                return dict(sums=f.bn_bwd_reduce(p["g"], p["s"], p["bn"], sums=p["rsum"]))
            return dict(sums=p["rsum"] + f.bn_bwd_reduce(p["g"], p["s"], p["bn"]))

        def out_bwd(p):
            small = acc(p["small4"])
            dm, ds, dg, db, cdm, cds = f.block_out_bwd(p["g"], p["s"], p["bn"], p["sums_s"], p["mask"], want_colsum_dm=True,
                                                        want_colsum_ds=True, **(dict(small=small) if own else {}))
            if not own:
                cdm, cds = p["small4"][2] + cdm, p["small4"][3] + cds
            return dict(dm=dm, ds=ds, dgamma=dg, dbeta=db, colsum_dm=cdm, colsum_ds=cds)

        def apply(p):
            ns = acc(p["nsum"])
            small = acc(p["small3"])
            dx, dg, db, cs = f.bn_bwd_apply(p["g"], p["x"], p["bnx"], p["sums_x"], mask=p["mask"], add=p["add"], want_colsum=True,
                                            next_s=p["s"], next_bn=p["bn"], next_sums=ns, **(dict(small=small) if own else {}))
            if not own:
                cs = p["small3"][2] + cs
            return dict(dx=dx, dgamma=dg, dbeta=db, colsum_dx=cs, next_sums=ns)
        return out_fwd, reduce, out_bwd, apply
    (fo, ro, bo, ao), (fr, rr, br, ar) = runs(ops), runs(TB)
    for mode, key in ((1, "bn"), (2, "bn2")):
        hh = dict(h, bn=h[key])
        guarded(arena, f"{tag}/block_out_fwd_bn{mode}", _pick(hh, "s", "m", "bn", "stats"), fo, fr, bars=dict(stats=st), inout=("stats",), ref64=r64)
        guarded(arena, f"{tag}/bn_relu_apply_bn{mode}", _pick(hh, "s", "bn"), lambda p: dict(out=ops.bn_relu_apply(p["s"], p["bn"])),
                lambda p: dict(out=TB.bn_relu_apply(p["s"], p["bn"])), ref64=r64)
    guarded(arena, f"{tag}/bn_bwd_reduce", _pick(h, "g", "s", "bn", "rsum"), ro, rr, bars=dict(sums=sm), inout=("rsum",), ref64=r64)
    for mask in h["masks"]:
        k = 0 if mask is None else mask.kind
        hh = dict(h, mask=mask)
        ds_ref = lambda: TB.block_out_bwd(h["g"], h["s"], h["bn"], h["sums_s"], mask)[1]
        small_bar = (2e-3, 2e-3) if f16 else None
        guarded(arena, f"{tag}/block_out_bwd_mask{k}", _pick(hh, "g", "s", "bn", "sums_s", "mask", "small4"), bo, br,
                bars=dict(colsum_ds=_colsum_zero_bar(ds_ref, h["small4"][3], f16, rows), dgamma=small_bar, dbeta=small_bar,
                          colsum_dm=small_bar),
                inout=("small4",), ref64=r64)
        dx_ref = lambda: TB.bn_bwd_apply(h["g"], h["x"], h["bnx"], h["sums_x"], mask=mask, add=h["add"])[0]
        # (the fp32 test_block_glue bounds colsum_dx on the scale of dx's column L1 norms; the bf16 one on the sum itself)
        cs_bar = (2e-3, 2e-3) if f16 else _colsum_zero_bar(dx_ref, h["small3"][2], False, rows)
        guarded(arena, f"{tag}/bn_bwd_apply_next_mask{k}", _pick(hh, "g", "x", "add", "s", "bn", "bnx", "sums_x", "mask", "small3", "nsum"), ao, ar,
                bars=dict(colsum_dx=cs_bar, next_sums=sm, dgamma=small_bar, dbeta=small_bar), inout=("small3", "nsum"), ref64=r64)
    cbar = (1e-4, 1e-4) if f16 else (1e-4, 1e-4 * math.sqrt(rows))
    guarded(arena, f"{tag}/colsum", _pick(h, "s"), lambda p: dict(out=ops.colsum(p["s"])), lambda p: dict(out=TB.colsum(p["s"])),
            bars=dict(out=cbar), ref64=r64)


@pytest.mark.parametrize("rows,c", [(37, 20), (3000, 1), (5, 640), (1000, 192), (64, 2008)])
def test_glue_fp32(arena, rows, c):
    """(37, 20) and (3000, 1): the scalar path; (64, 2008): the per-thread coefficient path above 640 channels.  All three mask
    kinds; statistics / sums / column sums accumulated onto non-zero starts; bn_bwd_apply in its fp32 next_s / next_bn /
    next_sums form (new: only the bf16 family had a test), vector and scalar (C = 20) instantiation"""
    _glue_case(arena, rows, c, torch.float32, 400 + rows + c)


@pytest.mark.parametrize("rows,c", [(7, 640), (300, 320)])
def test_glue_bf16(arena, rows, c):
    _glue_case(arena, rows, c, BF, 500 + rows + c, n=5 if rows % 5 == 0 else 1)


def test_bn_running_update(arena):
    gen = _gen(3)
    h = {}
    for i, (c, rows) in enumerate(((64, 1000), (20, 7), (640, 64))):
        x = torch.randn(rows, c, generator=gen).double() * 2 + 1
        h[f"sums{i}"], h[f"rm{i}"], h[f"rv{i}"] = torch.stack([x.sum(0), (x * x).sum(0)]), torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    counts = (1000, 7, 64)

    def run(f):
        def go(p):
            own = f is ops
            ent = [(p[f"sums{i}"], p[f"rm{i}"] if own else p[f"rm{i}"].clone(), p[f"rv{i}"] if own else p[f"rv{i}"].clone(), counts[i]) for i in range(3)]
            f.bn_running_update(ent)
            return {**{f"rm{i}": e[1] for i, e in enumerate(ent)}, **{f"rv{i}": e[2] for i, e in enumerate(ent)}}
        return go
    guarded(arena, "bn_running_update", h, run(ops), run(TB), bars={f"{k}{i}": (1e-5, 1e-5) for k in ("rm", "rv") for i in range(3)},
            inout=[f"{k}{i}" for k in ("rm", "rv") for i in range(3)], ref64=False)


# ---- latent kernels ----------------------------------------------------------------------------------------------------------
LATENT_NAMES = ("mus", "lvs", "jm", "jl", "z", "klds", "jd")


def _latent_case(arena, tag, mu, lv, eps, gs_seed, fwd_bars, bwd_bars):
    b = eps.shape[0]
    k = len(TB._active_subsets(mu))
    rs, w, norm = mixture_row_starts(b, k), kl_weights(k), float(b + 3)
    h = dict(mu=mu, lv=lv, eps=eps)
    guarded(arena, f"{tag}/fwd", h, lambda p: dict(zip(LATENT_NAMES, ops.latent_fwd(p["mu"], p["lv"], p["eps"], rs, w, norm))),
            lambda p: dict(zip(LATENT_NAMES, TB.latent_fwd(p["mu"], p["lv"], p["eps"], rs, w, norm))), bars={n: fwd_bars for n in LATENT_NAMES})
    gen = _gen(gs_seed)
    ref = TB.latent_fwd(mu, lv, eps, rs, w, norm)
    gs = [torch.randn(t.shape, generator=gen) for t in ref]
    for combo, g_use in (("all", gs), ("train", [None, None, None, None, gs[4], None, gs[6]])):
        hh = dict(h, gs=g_use)

        def run(f):
            def go(p):
                dmu, dlv = f.latent_bwd(p["mu"], p["lv"], p["eps"], rs, w, norm, *p["gs"])
                return {**{f"dmu{i}": t for i, t in enumerate(dmu)}, **{f"dlv{i}": t for i, t in enumerate(dlv)}}
            return go
        guarded(arena, f"{tag}/bwd_{combo}", hh, run(ops), run(TB), bars={f"{a}{i}": bwd_bars for a in ("dmu", "dlv") for i in range(3)})


@pytest.mark.parametrize("present", [(1, 1, 1), (1, 0, 0), (0, 1, 1)])
@pytest.mark.parametrize("b,d", [(7, 8), (65, 64)])
def test_latent(arena, present, b, d):
    gen = _gen(b * 100 + d + sum(present))
    mu = [torch.randn(b, d, generator=gen) if p else None for p in present]
    lv = [0.5 * torch.randn(b, d, generator=gen) if p else None for p in present]
    _latent_case(arena, f"latent{present}[{b}x{d}]", mu, lv, torch.randn(b, d, generator=gen), 1, (1e-4, 1e-5), (2e-4, 2e-5))


MIX_NAMES = ("sub_mu", "sub_lv", "comp_mu", "comp_lv", "joint_mu", "joint_lv", "z", "klds", "individual_divs", "joint_div", "pd_mu", "pd_lv")


def _np_bar(rtol, atol=None, atol_rel=None):
    def bar(name, got, ref):
        a = atol if atol is not None else atol_rel * max(float(ref.abs().max()), 1e-6)
        np.testing.assert_allclose(got.double().cpu().numpy(), ref.double().cpu().numpy(), rtol=BAR_SCALE * rtol, atol=BAR_SCALE * a, err_msg=name)
    return bar


def _mixture_case(arena, tag, method, mu, lv, eps, seed, wide=False):
    b = eps.shape[0]
    n = sum(t is not None for t in mu)
    c = n + (method == "jsd")
    w = kl_weights(n) if method == "moe" else [float(torch.tensor(1 / float(c)))] * c
    mrs, crs, norm = [mixture_row_starts(b, m) for m in (1, 2, 3)], mixture_row_starts(b, c), 64.0
    h = dict(mu=mu, lv=lv, eps=eps)
    bars = {nm: "eq" for nm in MIX_NAMES[:6]}
    bars.update({nm: _np_bar(2e-5, atol=1e-6) for nm in ("klds", "individual_divs", "joint_div")})
    bars.update({nm: _np_bar(1e-5, atol_rel=1e-5) for nm in ("z", "pd_mu", "pd_lv")})
    ref = TBM.latent_mixture_fwd(method, mu, lv, eps, mrs, crs, w, norm)
    # (the selection copies rows bit for bit: "eq" compares with the reference cast back to fp32)
    guarded(arena, f"{tag}/fwd", h, lambda p: dict(zip(MIX_NAMES, ops.latent_mixture_fwd(method, p["mu"], p["lv"], p["eps"], mrs, crs, w, norm))),
            lambda p: dict(zip(MIX_NAMES, TBM.latent_mixture_fwd(method, p["mu"], p["lv"], p["eps"], mrs, crs, w, norm))), bars=bars)
    gen = _gen(seed)
    gs = [None if r is None else torch.randn(r.shape, generator=gen) for r in ref]
    hh = dict(h, gs=gs)

    def run(f):
        def go(p):
            dmu, dlv = f.latent_mixture_bwd(method, p["mu"], p["lv"], p["eps"], mrs, crs, w, norm, *p["gs"])
            return {**{f"dmu{i}": t for i, t in enumerate(dmu)}, **{f"dlv{i}": t for i, t in enumerate(dlv)}}
        return go
    guarded(arena, f"{tag}/bwd", hh, run(ops), run(TBM), bars={f"{a}{i}": _np_bar(1e-4, atol_rel=1e-5) for a in ("dmu", "dlv") for i in range(3)})


@pytest.mark.parametrize("method", ["moe", "jsd"])
def test_latent_mixture(arena, method):
    for present in ((1, 1, 1), (1, 0, 0), (0, 1, 1)):
        for b, d in ((7, 8), (65, 64)):
            gen = _gen(1000 * b + d + 7 * sum(present))
            mu = [torch.randn(b, d, generator=gen) if p else None for p in present]
            lv = [0.7 * torch.randn(b, d, generator=gen) if p else None for p in present]
            _mixture_case(arena, f"mixture/{method}{present}[{b}x{d}]", method, mu, lv, torch.randn(b, d, generator=gen), 2)


def _style_case(arena, tag, smu, slv, eps, z, seed):
    b, d = z.shape
    norm = float(max(b, 2))
    h = dict(smu=smu, slv=slv, eps=eps, z=z)

    def fwd(f):
        def go(p):
            zcat, klds = f.latent_style_fwd(p["smu"], p["slv"], p["eps"], p["z"], norm)
            return {**{f"zcat{i}": t for i, t in enumerate(zcat)}, "klds": klds}
        return go
    dims = [0 if t is None else t.shape[1] for t in smu]

    def klds_bar(name, got, ref):      # the bar of test_style_gpu: 2e-6 relative x sqrt(S)
        for m in range(3):
            r = float(ref[m])
            assert abs(float(got[m]) - r) <= BAR_SCALE * (2e-6 * (abs(r) + 1e-3) * max(dims[m], 1) ** 0.5 + 1e-6), (name, m, float(got[m]), r)
    bars = {f"zcat{i}": _np_bar(1e-5, atol_rel=1e-5) for i in range(3)}
    bars["klds"] = klds_bar
    guarded(arena, f"{tag}/fwd", h, fwd(ops), fwd(TBS), bars=bars)
    gen = _gen(seed)
    hh = dict(h, g_zcat=[None if t is None else torch.randn(b, t.shape[1] + d, generator=gen) for t in smu], g_kl=torch.randn(3, generator=gen))
    del hh["z"]

    def bwd(f):
        def go(p):
            dmu, dlv, gz = f.latent_style_bwd(p["smu"], p["slv"], p["eps"], d, norm, p["g_zcat"], p["g_kl"])
            return {**{f"dmu{i}": t for i, t in enumerate(dmu)}, **{f"dlv{i}": t for i, t in enumerate(dlv)}, "g_z": gz}
        return go
    guarded(arena, f"{tag}/bwd", hh, bwd(ops), bwd(TBS), bars={k: _np_bar(1e-5, atol_rel=1e-5) for k in
                                                               [f"{a}{i}" for a in ("dmu", "dlv") for i in range(3)] + ["g_z"]})


def test_latent_style(arena):
    """style dims (1, 5, 32) in the three slots, all present and with a slot absent, B = 7 and 65"""
    for pres in ((1, 1, 1), (0, 1, 1), (1, 0, 0)):
        for b, d in ((7, 8), (65, 64)):
            gen = _gen(11 + b + sum(pres))
            mk = lambda s, f=1.0: torch.randn(b, s, generator=gen) * f
            dims = (1, 5, 32)
            _style_case(arena, f"style{pres}[{b}x{d}]", [mk(dims[m]) if pres[m] else None for m in range(3)],
                        [mk(dims[m], 0.5) if pres[m] else None for m in range(3)], [mk(dims[m]) if pres[m] else None for m in range(3)], mk(d), 3)


def _lhood_sample_case(arena, tag, mu, lv, eps, smu, slv, seps):
    d, s = mu.shape[1], smu.shape[1]
    names = ("zcat", "t_c", "t_s")

    def bar(dim):
        return lambda name, got, ref: np.testing.assert_allclose(got.double().cpu().numpy(), ref.double().cpu().numpy(), rtol=BAR_SCALE * 1e-5,
                                                                 atol=BAR_SCALE * (2e-5 * float(ref.abs().max()) + 1e-4 * dim), err_msg=name)
    guarded(arena, tag, dict(mu=mu, lv=lv, eps=eps, smu=smu, slv=slv, seps=seps),
            lambda p: dict(zip(names, ops.lhood_style_sample(p["mu"], p["lv"], p["eps"], p["smu"], p["slv"], p["seps"]))),
            lambda p: dict(zip(names, TBL.lhood_style_sample(p["mu"], p["lv"], p["eps"], p["smu"], p["slv"], p["seps"]))),
            bars=dict(zcat=_np_bar(2e-6, atol=1e-6), t_c=bar(d), t_s=bar(s)))


def test_lhood_estimator(arena):
    gen = _gen(3)
    u = lambda *shape, lo=-1.0, hi=1.0: (torch.rand(*shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float()
    for b, k, d, s in ((1, 6, 8, 1), (30, 10, 128, 32), (65, 1, 8, 5)):
        _lhood_sample_case(arena, f"lhood_style_sample[B{b} K{k} D{d} S{s}]", u(b, d, lo=-2, hi=2), u(b, d, lo=-6, hi=4), torch.randn(k, b, d, generator=gen),
                           u(b, s, lo=-2, hi=2), u(b, s, lo=-6, hi=4), torch.randn(k, b, s, generator=gen))
    for b, k in ((1, 6), (30, 10), (65, 1)):
        r = k * b
        h = dict(lp=[u(r, lo=-3000, hi=-1000) for _ in range(3)], t_c=u(r, lo=-30, hi=30), t_s=u(r, lo=-20, hi=20))
        for mask in (0, 5, 7):
            for with_ts in (True, False):
                hh = dict(h) if with_ts else _pick(h, "lp", "t_c")
                guarded(arena, f"lhood_estimates[B{b} K{k} mask{mask} ts{int(with_ts)}]", hh,
                        lambda p: dict(out=ops.lhood_estimates(p["lp"], p["t_c"], p.get("t_s"), k, mask)),
                        lambda p: dict(out=TBL.lhood_estimates(p["lp"], p["t_c"], p.get("t_s"), k, mask)), bars=dict(out=_np_bar(1e-6, atol=2e-3)))


# ---- likelihoods, vocabulary head, embedding ---------------------------------------------------------------------------------
def test_likelihoods(arena):
    gen = _gen(11)
    for n in (4099, 17):
        h = dict(xh=torch.randn(n, generator=gen), x=torch.rand(n, generator=gen), g=torch.tensor([0.33]))
        guarded(arena, f"laplace_nll_fwd[{n}]", _pick(h, "xh", "x"), lambda p: dict(out=ops.laplace_nll_fwd(p["xh"], p["x"], 0.75, 64.0)),
                lambda p: dict(out=TB.laplace_nll_fwd(p["xh"], p["x"], 0.75, 64.0)), bars=dict(out=(2e-6, 2e-6)))
        guarded(arena, f"laplace_nll_bwd[{n}]", h, lambda p: dict(dx=ops.laplace_nll_bwd(p["xh"], p["x"], p["g"], 0.75, 64.0)),
                lambda p: dict(dx=TB.laplace_nll_bwd(p["xh"], p["x"], p["g"], 0.75, 64.0)), bars=dict(dx=(1e-6, 1e-6)))
    for rows, v in ((33, 50), (3, 7000)):
        x = 3 * torch.randn(rows, v, generator=gen)
        y = TB.logsoftmax_fwd(x)
        ids = torch.randint(0, v, (rows,), generator=gen).float()
        ids[0], ids[1] = 0, v - 1                                   # boundary token ids
        h = dict(x=x, y=y, dy=torch.randn(rows, v, generator=gen), ids=ids, g=torch.tensor([0.7]))
        guarded(arena, f"logsoftmax_fwd[{rows}x{v}]", _pick(h, "x"), lambda p: dict(y=ops.logsoftmax_fwd(p["x"])),
                lambda p: dict(y=TB.logsoftmax_fwd(p["x"])), bars=dict(y=(1e-5, 1e-6)))
        guarded(arena, f"logsoftmax_bwd[{rows}x{v}]", _pick(h, "dy", "y"), lambda p: dict(dx=ops.logsoftmax_bwd(p["dy"], p["y"])),
                lambda p: dict(dx=TB.logsoftmax_bwd(p["dy"], p["y"])), bars=dict(dx=(1e-4, 1e-5)))
        guarded(arena, f"logsoftmax_bwd_bf16out[{rows}x{v}]", _pick(h, "dy", "y"), lambda p: dict(dx=ops.logsoftmax_bwd(p["dy"], p["y"], out_dtype=BF)),
                lambda p: dict(dx=TB.logsoftmax_bwd(p["dy"], p["y"], out_dtype=BF)), bars=dict(dx=(0, 1e-4)), ref64=False)
        guarded(arena, f"token_nll_fwd[{rows}x{v}]", _pick(h, "y", "ids"), lambda p: dict(out=ops.token_nll_fwd(p["y"], p["ids"], 8.0)),
                lambda p: dict(out=TB.token_nll_fwd(p["y"], p["ids"], 8.0)), bars=dict(out=(2e-6, 2e-6)))
        guarded(arena, f"token_nll_bwd[{rows}x{v}]", _pick(h, "ids", "g"), lambda p: dict(d=ops.token_nll_bwd(p["ids"], p["g"], (rows, v), 8.0)),
                lambda p: dict(d=TB.token_nll_bwd(p["ids"], p["g"], (rows, v), 8.0)), bars=dict(d=(1e-6, 1e-6)), ref64=False)
        guarded(arena, f"token_softmax_grad[{rows}x{v}]", _pick(h, "y", "ids", "g"), lambda p: dict(dx=ops.token_softmax_grad(p["y"], p["ids"], p["g"], 8.0)),
                lambda p: dict(dx=TB.token_softmax_grad(p["y"], p["ids"], p["g"], 8.0)), bars=dict(dx=(2e-6, 2e-6)))
    for b, L, F in ((3, 37, 5), (1, 1, 1)):
        h = dict(logp=torch.log_softmax(torch.randn(b, L, F, generator=gen), dim=-1), tgt=torch.rand(b, L, F, generator=gen), g=torch.tensor(0.37))
        guarded(arena, f"dense_nll_fwd[{b}x{L}x{F}]", _pick(h, "logp", "tgt"), lambda p: dict(out=ops.dense_nll_fwd(p["logp"], p["tgt"], float(b))),
                lambda p: dict(out=TB.dense_nll_fwd(p["logp"], p["tgt"], float(b))), bars=dict(out=(2e-6, 2e-6)))
        guarded(arena, f"dense_nll_bwd[{b}x{L}x{F}]", _pick(h, "tgt", "g"), lambda p: dict(d=ops.dense_nll_bwd(p["tgt"], p["g"], float(b))),
                lambda p: dict(d=TB.dense_nll_bwd(p["tgt"], p["g"], float(b))), bars=dict(d=(1e-6, 1e-7)))


def _head_inputs(b, L, V, dtype, seed):
    gen = _gen(seed)
    logits = (3.0 * torch.randn(b, L, V, generator=gen)).to(dtype)
    logits[..., V - 3:] = -1e30
    logits[0, 0, : V - 3] += 40.0
    ids = torch.randint(0, V - 3, (b, L), generator=gen).float()
    ids[0, 0], ids[-1, -1] = 0, V - 4                                # boundary token ids (the last real column)
    x64 = logits.double()
    return dict(logits=logits, ids=ids, g=torch.tensor([0.73]), lse=torch.logsumexp(x64, dim=-1).float()), x64


@pytest.mark.parametrize("V,dtype", [(8, torch.float32), (8, BF), (10240, BF)])
def test_vocabulary_head(arena, V, dtype):
    """lse_rows / token_nll_logits_fwd / token_softmax_grad_logits against double-precision torch on the same stored logits"""
    b, L = 2, 5
    h, x64 = _head_inputs(b, L, V, dtype, b * L + V)
    lse64 = torch.logsumexp(x64, dim=-1)
    guarded(arena, f"lse_rows[{V}]", _pick(h, "logits"), lambda p: dict(lse=ops.lse_rows(p["logits"])), dict(lse=lse64), bars=dict(lse=(2e-6, 2e-6)))
    guarded(arena, f"token_nll_logits_fwd[{V}]", _pick(h, "logits", "lse", "ids"),
            lambda p: dict(out=ops.token_nll_logits_fwd(p["logits"], p["lse"], p["ids"], float(b))),
            dict(out=TB.token_nll_logits_fwd(x64, h["lse"].double(), h["ids"], float(b))), bars=dict(out=(5e-6, 0)))
    ref = TB.token_softmax_grad_logits(x64, h["lse"].double(), h["ids"], h["g"].double(), float(b))
    bar = (1e-5, 2e-6) if dtype == torch.float32 else (lambda n, a, r: check(n, a.float(), r.to(BF).float(), rtol=1e-2, atol_rel=1e-4))
    guarded(arena, f"token_softmax_grad_logits[{V}]", h, lambda p: dict(dx=ops.token_softmax_grad_logits(p["logits"], p["lse"], p["ids"], p["g"], float(b))),
            dict(dx=ref), bars=dict(dx=bar))


@pytest.mark.parametrize("per_row", [7, 4099])
def test_logprob_rows(arena, per_row):
    gen = _gen(per_row)
    h = dict(xh=torch.rand(6, per_row, generator=gen), x=torch.rand(3, per_row, generator=gen))
    guarded(arena, f"laplace_logprob_rows[{per_row}]", h, lambda p: dict(out=ops.laplace_logprob_rows(p["xh"], p["x"], 0.75)),
            lambda p: dict(out=TB.laplace_logprob_rows(p["xh"], p["x"], 0.75)), bars=dict(out=(2e-6, 2e-6)))
    V = 9
    ids = torch.randint(0, V, (3, per_row), generator=gen).float()
    ids[0, 0], ids[-1, -1] = 0, V - 1
    h = dict(logp=torch.log_softmax(torch.randn(6, per_row, V, generator=gen), dim=-1), ids=ids)
    guarded(arena, f"token_logprob_rows[{per_row}]", h, lambda p: dict(out=ops.token_logprob_rows(p["logp"], p["ids"])),
            lambda p: dict(out=TB.token_logprob_rows(p["logp"], p["ids"])), bars=dict(out=(2e-6, 2e-6)))
    h = dict(logp=torch.log_softmax(torch.randn(6, per_row, 1, generator=gen) + torch.randn(6, 1, 1, generator=gen), dim=1), tgt=torch.rand(3, per_row, 1, generator=gen))
    guarded(arena, f"dense_logprob_rows[{per_row}]", h, lambda p: dict(out=ops.dense_logprob_rows(p["logp"], p["tgt"])),
            lambda p: dict(out=TB.dense_logprob_rows(p["logp"], p["tgt"])), bars=dict(out=(2e-6, 2e-6)))


def test_embedding(arena):
    """both families; ids include 0 (the padding index) and V - 1"""
    gen = _gen(4)
    for v, d, shape in ((50, 4, (4, 128)), (101, 64, (6, 16))):
        ids = torch.randint(0, v, shape, generator=gen).float()
        ids[:, :3] = 0
        ids[:, -1] = v - 1
        for dtype in (torch.float32, BF):
            h = dict(ids=ids, table=torch.randn(v, d, generator=gen), gout=torch.randn(*shape, d, generator=gen).to(dtype))
            guarded(arena, f"embedding_fwd[{v}x{d}]{dtype}", _pick(h, "ids", "table"), lambda p: dict(out=ops.embedding_fwd(p["ids"], p["table"], out_dtype=dtype)),
                    lambda p: dict(out=TB.embedding_fwd(p["ids"], p["table"], out_dtype=dtype)), bars=dict(out="eq"), ref64=False)
            guarded(arena, f"embedding_bwd[{v}x{d}]{dtype}", _pick(h, "ids", "gout"), lambda p: dict(d=ops.embedding_bwd(p["ids"], p["gout"], v, 0)),
                    lambda p: dict(d=TB.embedding_bwd(p["ids"], p["gout"], v, 0)), bars=dict(d=(1e-4, 1e-5)), ref64=False)


def test_adam_step(arena):
    """sizes 1, 3, 5 and 4097 (below / across the 4-element vector and the 4096-element chunk), one with a bf16 copy"""
    gen = _gen(12)
    sizes = (1, 3, 5, 4097)
    h = dict(p=[torch.randn(n, generator=gen) for n in sizes], g=[torch.randn(n, generator=gen) * (3.0 if i % 2 else 0.01) for i, n in enumerate(sizes)],
             m=[0.1 * torch.randn(n, generator=gen) for n in sizes], v=[0.1 * torch.rand(n, generator=gen) for n in sizes],
             p16=torch.zeros(4097, dtype=BF), step=torch.tensor(2.0), coef=torch.zeros(2))

    def run(f):
        def go(p):
            own = f is ops
            c = (lambda t: t) if own else (lambda t: t.clone())
            ps, ms, vs, step, p16 = [c(t) for t in p["p"]], [c(t) for t in p["m"]], [c(t) for t in p["v"]], c(p["step"]), c(p["p16"])
            f.adam_step(ps, p["g"], ms, vs, step, 2e-3, 0.9, 0.999, 1e-8, p["coef"], lowp=[None, None, None, p16])
            out = {f"p{i}": t for i, t in enumerate(ps)}
            out.update({f"m{i}": t for i, t in enumerate(ms)})
            out.update({f"v{i}": t for i, t in enumerate(vs)})
            out.update(step=step.reshape(1))
            return out
        return go
    bars = {f"{k}{i}": (2e-6, 2e-7) for k in "pmv" for i in range(4)}
    guarded(arena, "adam_step", h, run(ops), run(TB), bars=bars, inout=("p", "m", "v", "p16", "step", "coef"), ref64=False)


def test_adam_step_bf16_copy(arena):
    """the p16 copy is the updated parameter rounded once"""
    gen = _gen(13)
    n = 4097
    arena.reset()
    p, g, m, v = (arena.place(t, name=k) for k, t in (("p", torch.randn(n, generator=gen)), ("g", torch.randn(n, generator=gen)),
                                                       ("m", torch.zeros(n)), ("v", torch.zeros(n))))
    p16 = arena.place(torch.zeros(n, dtype=BF), name="p16")
    step, coef = arena.place(torch.zeros(1), name="step"), arena.place(torch.zeros(2), name="coef")
    ops.adam_step([p], [g], [m], [v], step, 2e-3, 0.9, 0.999, 1e-8, coef, lowp=[p16])
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert float(step) == 1.0 and torch.equal(p16.cpu(), p.cpu().to(BF))


@pytest.mark.parametrize("n,d,l", [(33, 1, 1), (500, 128, 3), (64, 256, 2)])
def test_logreg(arena, n, d, l):
    """the fit against the float64 optimum of the same problem: |grad f|_inf <= 1e-4 N in float64 at the returned W (bar (a) of
    tests/test_lr_eval_gpu.py), predictions equal to the sign of the float64 decision values away from the boundary"""
    gen = _gen(n + d)
    s = 2
    x = torch.randn(s, n, d, generator=gen)
    y = (torch.rand(n, l, generator=gen) < 0.5).float()
    y[0], y[1] = 0.0, 1.0                                            # both classes in every label column
    h = dict(x=x, y=y)

    def grad_bar(name, got, ref):
        gi = LU.grad_inf(got.double().cpu().numpy(), x.numpy(), y.numpy())
        assert np.isfinite(gi).all() and (gi <= 1e-4 * n).all(), (name, gi.max())
    got = guarded(arena, f"logreg_fit[{n}x{d}x{l}]", h, lambda p: dict(zip(("w", "info"), ops.logreg_fit(p["x"], p["y"]))),
                  lambda p: dict(w=TBLR.logreg_fit(p["x"], p["y"])[0]), bars=dict(w=grad_bar), ref64=False)
    w = got["w"].cpu()
    xt = torch.randn(s, 17, d, generator=gen)
    dec64 = TBLR.logreg_predict(xt, w, want_decision=True)[1]

    def pred_bar(name, got, ref):
        far = dec64.abs() > 1e-4 * (1 + dec64.abs().max())
        assert torch.equal(got.cpu()[far], (dec64 > 0).float()[far]), name
    guarded(arena, f"logreg_predict[{n}x{d}x{l}]", dict(xt=xt, w=w), lambda p: dict(zip(("pred", "dec"), ops.logreg_predict(p["xt"], p["w"], want_decision=True))),
            dict(pred=dec64, dec=dec64), bars=dict(pred=pred_bar, dec=(1e-5, 1e-5)))


# ---- alignment ---------------------------------------------------------------------------------------------------------------
def test_misaligned_fp32_operands_take_the_scalar_path(arena):
    """one operand at a time 4 bytes off a 16-byte boundary: the fp32 glue, conv forward / input gradient / weight gradient and
    the Laplace kernels give the results of the aligned call (same references, same bars), guards intact"""
    g = _geom("odd_grid_T_96to32")
    h = _conv32_inputs(g, 31)
    fwd_in, dg_in, wg_in = _pick(h, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns"), _pick(h, "x", "wp", "dy", "bn", "sums"), _pick(h, "x", "dy", "bn")
    fref, dref, wref = _fwd_ref(g)(fwd_in), _dgrad_ref(g)(dg_in), _wgrad_ref(g)(wg_in)
    for op in ("x", "wp", "mask.mask", "bias"):
        guarded(arena, f"misaligned/{op}/fwd", fwd_in, _fwd_call(g), fref, bars=dict(stats=STATS), inout=("stats",), misalign={op: 4})
    for op in ("dy", "wp", "x"):
        guarded(arena, f"misaligned/{op}/dgrad", dg_in, _dgrad_call(g), dref, bars=dict(sums=SUMS), inout=("sums",), misalign={op: 4})
    for op in ("x", "dy"):
        guarded(arena, f"misaligned/{op}/wgrad", wg_in, _wgrad_call(g), wref, misalign={op: 4})
        guarded(arena, f"misaligned/{op}/wgrad_bn", wg_in, _wgrad_call(g, True), _wgrad_ref(g, True)(wg_in), misalign={op: 4})
    hg, rows = _glue_inputs(1000, 192, torch.float32, 32)
    hg["mask"] = hg["masks"][2]
    for op in ("s", "m"):
        guarded(arena, f"misaligned/{op}/block_out_fwd", _pick(hg, "s", "m", "bn", "stats"),
                lambda p: dict(out=ops.block_out_fwd(p["s"], p["m"], p["bn"], out_stats=p["stats"]), stats=p["stats"]),
                lambda p: (lambda st: dict(out=TB.block_out_fwd(p["s"], p["m"], p["bn"], out_stats=st), stats=st))(p["stats"].clone()),
                bars=dict(stats=STATS), inout=("stats",), misalign={op: 4})
    guarded(arena, "misaligned/s/bn_relu_apply", _pick(hg, "s", "bn"), lambda p: dict(out=ops.bn_relu_apply(p["s"], p["bn"])),
            lambda p: dict(out=TB.bn_relu_apply(p["s"], p["bn"])), misalign={"s": 4})
    for op in ("g", "s"):
        guarded(arena, f"misaligned/{op}/bn_bwd_reduce", _pick(hg, "g", "s", "bn"), lambda p: dict(sums=ops.bn_bwd_reduce(p["g"], p["s"], p["bn"])),
                lambda p: dict(sums=TB.bn_bwd_reduce(p["g"], p["s"], p["bn"])), bars=dict(sums=SUMS), misalign={op: 4})
    for op in ("g", "x", "add", "mask.mask"):
        guarded(arena, f"misaligned/{op}/bn_bwd_apply", _pick(hg, "g", "x", "add", "bnx", "sums_x", "mask"),
                lambda p: dict(dx=ops.bn_bwd_apply(p["g"], p["x"], p["bnx"], p["sums_x"], mask=p["mask"], add=p["add"])[0]),
                lambda p: dict(dx=TB.bn_bwd_apply(p["g"], p["x"], p["bnx"], p["sums_x"], mask=p["mask"], add=p["add"])[0]), misalign={op: 4})
    for op in ("g", "s"):
        guarded(arena, f"misaligned/{op}/block_out_bwd", _pick(hg, "g", "s", "bn", "sums_s", "mask"),
                lambda p: dict(zip(("dm", "ds"), ops.block_out_bwd(p["g"], p["s"], p["bn"], p["sums_s"], p["mask"])[:2])),
                lambda p: dict(zip(("dm", "ds"), TB.block_out_bwd(p["g"], p["s"], p["bn"], p["sums_s"], p["mask"])[:2])), misalign={op: 4})
    guarded(arena, "misaligned/s/colsum", _pick(hg, "s"), lambda p: dict(out=ops.colsum(p["s"])), lambda p: dict(out=TB.colsum(p["s"])),
            bars=dict(out=(1e-4, 1e-4 * math.sqrt(rows))), misalign={"s": 4})
    gen = _gen(33)
    hl = dict(xh=torch.randn(4100, generator=gen), x=torch.rand(4100, generator=gen), g=torch.tensor([0.33]))
    for op in ("xh", "x"):
        guarded(arena, f"misaligned/{op}/laplace_nll_fwd", _pick(hl, "xh", "x"), lambda p: dict(out=ops.laplace_nll_fwd(p["xh"], p["x"], 0.75, 64.0)),
                lambda p: dict(out=TB.laplace_nll_fwd(p["xh"], p["x"], 0.75, 64.0)), bars=dict(out=(2e-6, 2e-6)), misalign={op: 4})
        guarded(arena, f"misaligned/{op}/laplace_nll_bwd", hl, lambda p: dict(dx=ops.laplace_nll_bwd(p["xh"], p["x"], p["g"], 0.75, 64.0)),
                lambda p: dict(dx=TB.laplace_nll_bwd(p["xh"], p["x"], p["g"], 0.75, 64.0)), bars=dict(dx=(1e-6, 1e-6)), misalign={op: 4})
        hr = dict(xh=hl["xh"].view(4, 1025), x=hl["x"].view(4, 1025)[:2].clone())
        guarded(arena, f"misaligned/{op}/laplace_logprob_rows", hr, lambda p: dict(out=ops.laplace_logprob_rows(p["xh"], p["x"], 0.75)),
                lambda p: dict(out=TB.laplace_logprob_rows(p["xh"], p["x"], 0.75)), bars=dict(out=(2e-6, 2e-6)), misalign={op: 4})


def test_misaligned_operands_are_refused_where_there_is_no_scalar_path(arena):
    """bf16 conv and glue, conv_fwd(mix=) in fp32, the block-front kernels and lse_rows: MOPOE_ERR_ARG, nothing launched (every
    result the wrapper allocated is still pure poison)"""
    g = dict(GEOMS16)["odd_grid_k4s2p1_b3"]
    h = _conv16_inputs(g, 41)
    fwd_in, dg_in, wg_in = _pick(h, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns"), _pick(h, "x", "wp", "dy", "bn", "sums"), _pick(h, "x", "dy", "bn")
    for op in ("x", "wp"):
        guarded(arena, f"refused/{op}/fwd16", fwd_in, _fwd16(g, True, False)[0], None, misalign={op: 8}, raises=True)
    guarded(arena, "refused/sres/fwd_mix16", fwd_in, _fwd16(g, True, True)[0], None, misalign={"sres": 8}, raises=True)
    for op in ("dy", "wp", "x"):
        guarded(arena, f"refused/{op}/dgrad16", dg_in, _dgrad16(g, True)[0], None, misalign={op: 8}, raises=True)
    for op in ("x", "dy"):
        guarded(arena, f"refused/{op}/wgrad16", wg_in, _wgrad_call(g), None, misalign={op: 8}, raises=True)
    hg, _rows = _glue_inputs(300, 320, BF, 42, n=5)
    hg["mask"] = hg["masks"][1]
    for op in ("s", "m"):
        guarded(arena, f"refused/{op}/block_out_fwd16", _pick(hg, "s", "m", "bn"), lambda p: dict(out=ops.block_out_fwd(p["s"], p["m"], p["bn"])), None,
                misalign={op: 8}, raises=True)
    guarded(arena, "refused/s/bn_relu_apply16", _pick(hg, "s", "bn"), lambda p: dict(out=ops.bn_relu_apply(p["s"], p["bn"])), None, misalign={"s": 8}, raises=True)
    for op in ("g", "s"):
        guarded(arena, f"refused/{op}/bn_bwd_reduce16", _pick(hg, "g", "s", "bn"), lambda p: dict(sums=ops.bn_bwd_reduce(p["g"], p["s"], p["bn"])), None,
                misalign={op: 8}, raises=True)
        guarded(arena, f"refused/{op}/block_out_bwd16", _pick(hg, "g", "s", "bn", "sums_s", "mask"),
                lambda p: dict(dm=ops.block_out_bwd(p["g"], p["s"], p["bn"], p["sums_s"], p["mask"])[0]), None, misalign={op: 8}, raises=True)
    for op in ("g", "x", "add"):
        guarded(arena, f"refused/{op}/bn_bwd_apply16", _pick(hg, "g", "x", "add", "bnx", "sums_x", "mask"),
                lambda p: dict(dx=ops.bn_bwd_apply(p["g"], p["x"], p["bnx"], p["sums_x"], mask=p["mask"], add=p["add"])[0]), None, misalign={op: 8}, raises=True)
    guarded(arena, "refused/s/colsum16", _pick(hg, "s"), lambda p: dict(out=ops.colsum(p["s"])), None, misalign={"s": 8}, raises=True)
    # fp32: the residual mix has no scalar path
    g32 = _geom("odd_grid_T_96to32")
    h32 = _conv32_inputs(g32, 43)
    f32_in = _pick(h32, "x", "wp", "bias", "bn", "mask", "stats", "sres", "bns")
    for op in ("x", "wp", "sres"):
        guarded(arena, f"refused/{op}/fwd_mix32", f32_in, _fwd_call(g32, mix=True), None, misalign={op: 4}, raises=True)
    for family, dtype, off in (("fp32", torch.float32, 4), ("bf16", BF, 8)):
        hf = _front_inputs(dtype)
        s_o, a_o, b_o = _front_runs(ops)
        for op in ("x", "w1"):
            guarded(arena, f"refused/{op}/front_stats/{family}", _pick(hf, "x", "w1", "bias", "bn1", "mask", "stats"), s_o, None, misalign={op: off}, raises=True)
            guarded(arena, f"refused/{op}/front_apply/{family}", _pick(hf, "x", "w1", "bias", "bn1", "bn2", "mask"), a_o, None, misalign={op: off}, raises=True)
        for op in ("x", "w1", "dh2"):
            guarded(arena, f"refused/{op}/front_bwd/{family}", hf, b_o, None, misalign={op: off}, raises=True)
    for dtype, off in ((torch.float32, 4), (BF, 8)):
        hh, _ = _head_inputs(2, 5, 8, dtype, 44)
        guarded(arena, f"refused/lse_rows/{dtype}", _pick(hh, "logits"), lambda p: dict(lse=ops.lse_rows(p["logits"])), None, misalign={"logits": off}, raises=True)


# ---- aliasing the header allows ------------------------------------------------------------------------------------------------
def test_documented_aliasing_is_bit_equal_to_out_of_place(arena):
    """logsoftmax_fwd (y may alias x), logsoftmax_bwd (dx may alias dy; fp32 -- the bf16out form writes another type and has
    no in-place form: run out of place twice, bit-equal), token_softmax_grad_logits (dx may alias logits) in bf16"""
    gen = _gen(21)
    x = 3 * torch.randn(33, 50, generator=gen)
    dy = torch.randn(33, 50, generator=gen)

    def both(tag, h, name, out_of_place, in_place):
        a = guarded(arena, f"alias/{tag}/out_of_place", h, lambda p: dict(r=out_of_place(p)), {})["r"].clone()
        b = guarded(arena, f"alias/{tag}/in_place", h, lambda p: dict(r=in_place(p)), {}, inout=(name,))["r"]
        assert torch.equal(_bits(a), _bits(b)), tag
    both("logsoftmax_fwd", dict(x=x), "x", lambda p: ops.logsoftmax_fwd(p["x"]), lambda p: ops.logsoftmax_fwd(p["x"], inplace=True))
    y = TB.logsoftmax_fwd(x)
    both("logsoftmax_bwd", dict(dy=dy, y=y), "dy", lambda p: ops.logsoftmax_bwd(p["dy"], p["y"]), lambda p: ops.logsoftmax_bwd(p["dy"], p["y"], inplace=True))
    both("logsoftmax_bwd_bf16out", dict(dy=dy, y=y), "dy", lambda p: ops.logsoftmax_bwd(p["dy"], p["y"], out_dtype=BF),
         lambda p: ops.logsoftmax_bwd(p["dy"], p["y"], inplace=True, out_dtype=BF))
    for V in (8, 10240):
        h, _ = _head_inputs(2, 5, V, BF, 22 + V)
        both(f"token_softmax_grad_logits[{V}]", h, "logits", lambda p: ops.token_softmax_grad_logits(p["logits"], p["lse"], p["ids"], p["g"], 2.0),
             lambda p: ops.token_softmax_grad_logits(p["logits"], p["lse"], p["ids"], p["g"], 2.0, inplace=True))


# ---- BatchNorm at shifted means ------------------------------------------------------------------------------------------------
def _relerr(a, ref64):
    return float((a.double().cpu() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("rows", HS.BN_SHIFT_ROWS)
@pytest.mark.parametrize("r", HS.BN_SHIFTS)
@pytest.mark.parametrize("narrow", [False, True])
def test_bn_shifted_means(arena, rows, r, narrow):
    """rows x 64 activations randn + r (narrow: channel 5 scaled by 1e-2 around the same mean): the statistics conv_fwd
    accumulates, conv_fwd with that BatchNorm on load, bn_relu_apply, bn_bwd_reduce, bn_bwd_apply and bn_running_update
    against an fp64 evaluation of the same stored inputs, beside torch.nn.functional.batch_norm and its autograd in fp32 on
    the CPU against the same fp64.  Gate for r <= 30: kernel error <= 4 x reference error + the floor of `check`
    (2e-4 of the tensor's scale; 1e-4 for the statistics; 1e-5 for the running statistics); r = 100 is logged only."""
    c = 64
    h = HS.bn_shift_inputs(rows, c, r, narrow)
    x, dy, gamma, beta, w1 = h["x"], h["dy"], h["gamma"], h["beta"], h["w1"]
    g1 = Geom(1, rows, 1, rows, 1, c, c, 1, 1, 1, 1, 0, 0, False)
    ref = HS.bn_reference_errors(h)                     # fp64 values and the fp32 reference's errors
    t64 = ref["fp64"]
    tag = f"bn_shift[{rows}x{c} r={r}{' narrow' if narrow else ''}]"
    # the statistics: an identity 1x1 conv writes y = x and accumulates {sum, sumsq} of it
    eye = torch.eye(c).view(1, c, c)
    got = guarded(arena, f"{tag}/stats", dict(x=x.view(g1.in_shape), eye=eye, stats=torch.zeros(2, c, dtype=torch.float64)),
                  lambda p: dict(y=ops.conv_fwd(p["x"], p["eye"], g1, out_stats=p["stats"]), stats=p["stats"]), {}, inout=("stats",))
    assert torch.equal(got["y"].cpu().view(rows, c), x)
    stats = got["stats"].cpu().clone()
    mean_k = stats[0] / rows
    var_k = (stats[1] / rows - mean_k * mean_k).clamp_min(0)
    bn = Bn(gamma, beta, 1, sums=stats, count=rows)     # the kernels' OWN statistics feed every kernel below
    run = guarded(arena, f"{tag}/kernels", dict(x=x, dy=dy, w1=w1, bn=bn, rm=torch.zeros(c), rv=torch.ones(c)),
                  lambda p: dict(xhat_relu=ops.bn_relu_apply(p["x"], p["bn"]),
                                 conv=ops.conv_fwd(p["x"].view(g1.in_shape), p["w1"], g1, bn_in=p["bn"]),
                                 sums=ops.bn_bwd_reduce(p["dy"], p["x"], p["bn"]),
                                 rm=(ops.bn_running_update([(p["bn"].sums, p["rm"], p["rv"], rows)]), p["rm"])[1], rv=p["rv"]),
                  {}, inout=("rm", "rv"))
    run = {k: v.clone() for k, v in run.items()}          # (arena views: the next guarded call poisons them again)
    run["run"] = torch.stack([run["rm"], run["rv"]])
    sums = run["sums"]
    dx = guarded(arena, f"{tag}/bn_bwd_apply", dict(x=x, dy=dy, bn=bn, sums=sums.cpu()),
                 lambda p: dict(dx=ops.bn_bwd_apply(p["dy"], p["x"], p["bn"], p["sums"])[0]), {})["dx"]
    _log(f"{tag}/derived (not gated): mean_err={_relerr(mean_k, t64['mean']):.3e} (reference {ref['ref_err']['mean']:.3e}) "
         f"var_err={float(((var_k - t64['var']).abs() / t64['var']).max()):.3e} (reference {ref['ref_err']['var']:.3e})")
    kernel = dict(conv_fwd_stats=_relerr(stats, t64["stats"]),
                  bn_relu_apply=_relerr(run["xhat_relu"], t64["act"]), conv_bn_on_load=_relerr(run["conv"].view(rows, c), t64["conv"]),
                  bn_bwd_reduce=_relerr(run["sums"], t64["sums"]), bn_bwd_apply=_relerr(dx, t64["dx"]),
                  bn_running_update=_relerr(run["run"], t64["run"]))
    floor = HS.BN_FLOOR
    bad = []
    for k, e in kernel.items():
        re_ = ref["ref_err"][k]
        _log(f"{tag}/{k}: kernel_err={e:.3e} reference_err={re_:.3e} ratio={e / max(re_, 1e-30):.2f}" + ("" if r <= HS.BN_GATED_SHIFT else " (logged, not gated)"))
        if r <= HS.BN_GATED_SHIFT and not e <= 4 * re_ + floor[k]:
            bad.append((k, e, re_))
    assert not bad, (tag, bad)


# ---- degenerate channels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_c20", "vector_c64"])
@pytest.mark.parametrize("case", HS.DEGENERATE_CASES)
def test_degenerate_channels(arena, name, case):
    """a constant column (variance 0: eps decides), gamma == 0 under modes 1 and 3 (dgrad with xin = the activation), rvar == 0
    under mode 2 -- forward, bn_bwd_apply and conv_dgrad with relu_bn, against the fp64 evaluation at the existing bars"""
    g = _geom("ragged_c20") if name == "ragged_c20" else Geom(3, 8, 8, 16, 16, 64, 64, 4, 4, 2, 2, 1, 1, False)
    h = HS.degenerate_inputs(g, case)
    bn, x = h["bn"], h["x"]
    fwd_in = _pick(h, "x", "wp", "bias", "bn")
    guarded(arena, f"degenerate/{name}/{case}/fwd", fwd_in, lambda p: dict(y=ops.conv_fwd(p["x"], p["wp"], g, bn_in=p["bn"], bias=p["bias"])),
            lambda p: dict(y=TB.conv_fwd(p["x"], p["wp"], g, bn_in=p["bn"], bias=p["bias"])))
    guarded(arena, f"degenerate/{name}/{case}/bn_relu_apply", _pick(h, "x", "bn"), lambda p: dict(a=ops.bn_relu_apply(p["x"], p["bn"])),
            lambda p: dict(a=TB.bn_relu_apply(p["x"], p["bn"])))
    guarded(arena, f"degenerate/{name}/{case}/bn_bwd_apply", _pick(h, "gx", "x", "bn", "sums_x"),
            lambda p: dict(zip(("dx", "dgamma", "dbeta"), ops.bn_bwd_apply(p["gx"], p["x"], p["bn"], p["sums_x"])[:3])),
            lambda p: dict(zip(("dx", "dgamma", "dbeta"), TB.bn_bwd_apply(p["gx"], p["x"], p["bn"], p["sums_x"])[:3])))
    xin, rb = (h["act"], Bn(bn.gamma, bn.beta, 3, sums=bn.sums, count=bn.count)) if case == "gamma0_mode3" else (x, bn)
    dg_in = dict(dy=h["dy"], wp=h["wp"], xin=xin, bn=rb, sums=_prefill((2, g.Cin), _gen(6)))

    def dgrad(f):
        def go(p):
            s = p["sums"] if f is ops else p["sums"].clone()
            return dict(dx=f.conv_dgrad(p["dy"], p["wp"], g, relu_bn=p["bn"], xin=p["xin"], bwd_sums=s), sums=s)
        return go
    guarded(arena, f"degenerate/{name}/{case}/dgrad", dg_in, dgrad(ops), dgrad(TB), bars=dict(sums=SUMS), inout=("sums",))


# ---- latent kernels at wide log-variances ------------------------------------------------------------------------------------------
def test_latent_kernels_at_wide_logvariances(arena):
    """mu ~ 3 randn, logvar uniform in the range tests/test_arena_cpu.py pins (hostile_sets.WIDE_LOGVAR): latent_fwd / bwd, the
    mixture pair, the style pair and lhood_style_sample at the bars of their present tests"""
    lo, hi = HS.WIDE_LOGVAR
    for b, d in ((7, 8), (65, 64)):
        mu, lv, eps = HS.wide_latent_inputs(b, d, (1, 1, 1))
        _latent_case(arena, f"wide/latent[{b}x{d}]", mu, lv, eps, 5, (1e-4, 1e-5), (2e-4, 2e-5))
        for method in ("moe", "jsd"):
            _mixture_case(arena, f"wide/mixture/{method}[{b}x{d}]", method, mu, lv, eps, 6)
        smu, slv, seps, z = HS.wide_style_inputs(b, d, (1, 5, 32))
        _style_case(arena, f"wide/style[{b}x{d}]", smu, slv, seps, z, 7)
        k = 6
        gen = _gen(8 + b)
        _lhood_sample_case(arena, f"wide/lhood_style_sample[{b}x{d}]", mu[0], lv[0], torch.randn(k, b, d, generator=gen), smu[2], slv[2],
                           torch.randn(k, b, 32, generator=gen))


# ---- the table of the docstring against what was really launched (last: it reads what the tests above recorded) --------------------
def test_every_row_of_the_table_was_called_by_its_test():
    """each entry point of the table was handed to the library, inside outputs_in, by a case of the test its row names.  Rows
    whose test did not run in this session (a -k selection) are not judged, and a selection of some cases of a test may miss a row
    another case covers; a full run of the file judges every row"""
    table = coverage_table()
    assert len(table) > 55
    judged = {fn: test for fn, test in table.items() if test in CALLED_BY_TEST}
    missing = sorted(f"{fn} (by {test})" for fn, test in judged.items() if fn not in CALLED_BY_TEST[test])
    _log(f"guarded: {len(judged)} of {len(table)} table rows judged against the recorded calls, {len(missing)} missing")
    assert not missing, missing
