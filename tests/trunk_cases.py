"""TEST INFRASTRUCTURE: two-block residual chains through mimic_amd.trunk (trunk_forward, trunk_backward,
apply_running_updates) against oracle/mopoe_ref._resblock chained under autograd, element by element.

A case is small enough that NO BN -> ReLU pre-activation of the fp64 reference lies within M = 5e-5 of zero (asserted from the
reference alone, for the case's fixed seed, in every mode), so two correct fp32 implementations agree on every ReLU mask and every
tensor of the chain can be compared element-wise: nothing is trimmed, sampled or set aside.  The yardstick of a tensor is the
oracle's own fp32-vs-fp64 deviation on that tensor (`Reference.dev`), measured on the scale of the tensor.

tests/test_trunk_chain_cpu.py runs the chains on tests/torch_backend.py (trunk.py's chain rule with emulated ops),
tests/test_trunk_chain_gpu.py on the HIP kernels; tests/tools/trunk_seeds.py finds the seeds.  Nothing here touches a GPU."""
from __future__ import annotations

import copy
import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

import mopoe_ref as R
from mimic_amd import ops, trunk
from mimic_amd.layout import ResBlockParams, pack_weight, unpack_weight
from mimic_amd.ops import Geom

M = 5e-5                      # every ReLU input of the fp64 reference is at least this far from zero (5 x the 1e-5 max bar
#                               the project sets on split-bf16 plain-operand tiles)
MODES = ("train_nodrop", "train", "eval")
BF16 = torch.bfloat16
# the oracle's fp32 run cannot be told from luck below one fp32 rounding step of the tensor's scale: a result stored in fp32 is
# off by up to 2^-24 of its own size before anything was computed.  Deviations are floored there, so that a tensor the fp32
# oracle happened to hit exactly does not ask the kernels for more than the format holds.
DEV_FLOOR = 2.0 ** -23
# ... nor is it a yardstick where it strays far: a train-mode BatchNorm over a handful of rows with a nearly constant channel
# (the 3 rows a B = 3 chain ends on) multiplies ONE rounding error by 1 / sigma, the oracle's deviation is then a single draw of
# that error and any other fp32 implementation's is another.  A seed counts only if the fp32 oracle stays within 16 fp32
# rounding steps of fp64 on every tensor (well-conditioned chains measure 4e-7 ... 1.2e-6); like M this is asserted on the
# reference alone, and it can only tighten what the code under test is held to.
DEV_MAX = 2.0 ** -19


@dataclass(frozen=True)
class Case:
    name: str
    batch: int
    twod: bool                      # 2-D blocks (channel masks) or 1-D blocks (element masks)
    transposed: bool
    size: int                       # H = W (2-D) or L (1-D) of the chain's input
    chans: Tuple[int, int, int]     # channels in, between the blocks, out
    plan: Tuple[Tuple[int, int], ...]   # (stride, padding) of each block's k4 conv, as the reference builds it
    main_bias: bool
    seed: int                       # tests/tools/trunk_seeds.py: the first seed that meets M and DEV_MAX in all three modes
    fronts: Tuple[Tuple[int, ...], ...]   # blocks whose backward runs ops.block_front_bwd by default, per mode of MODES
    mix: bool = True                # the residual mix rides in conv2's epilogue (fp32: channel counts that are multiples of 4)


# Written out by hand from the rules of ops.block_front_supported (64 -> 64 channels, rows % 32 == 0, a channel mask only on whole
# 32-row tiles per sample): `fronts` is what the recorder must see, not what the code under test says about itself.
CASES = [
    # B = 2, 8x8 -> 4x4 -> 2x2: block 0 has 128 rows (64 per sample), block 1 has 32 rows (16 per sample: no front under dropout)
    Case("enc2d", 2, True, False, 8, (64, 64, 96), ((2, 1), (2, 1)), True, 0, ((0, 1), (0,), (0, 1))),
    # B = 2, 4x4 -> 8x8 -> 16x16: block 0 has 32 rows (16 per sample), block 1 has 128 rows
    Case("dec2d", 2, True, True, 4, (64, 64, 32), ((2, 1), (2, 1)), True, 31, ((0, 1), (1,), (0, 1))),
    # B = 8, 1x1 -> 4x4 -> 8x8: the first block is the k4 s1 p0 transposed conv on one pixel that DecoderImg runs as s4 (16 one-tap
    # phases) on 8 rows of 96 channels: no front; block 1 has 128 rows of 64 channels, 16 per sample
    Case("dec_from1", 8, True, True, 1, (96, 64, 32), ((1, 0), (2, 1)), True, 7, ((1,), (), (1,))),
    Case("text1d", 2, False, False, 16, (128, 128, 192), ((2, 1), (2, 1)), True, 1, ((), (), ())),
    Case("textT1d", 2, False, True, 4, (192, 128, 128), ((2, 1), (2, 1)), True, 3, ((), (), ())),
    # B = 3, 6x6 -> 3x3 -> 1x1, 6 -> 10 -> 7 channels: no vector path, drop2(conv2) is written out and mixed by block_out_fwd.  The
    # second block's k4 conv takes 3x3 to 1x1 with stride 3: the library wants the big grid to be a multiple of the stride
    Case("ragged", 3, True, False, 6, (6, 10, 7), ((2, 1), (3, 1)), True, 0, ((), (), ()), mix=False),
    # 64 channels but 48 and 12 rows: the streaming front must be refused on the row count alone
    Case("rows48", 3, True, False, 4, (64, 64, 64), ((2, 1), (2, 1)), True, 9, ((), (), ())),
    # the image networks' blocks: no bias on conv1 / conv2 (the front's dbias pointer is NULL, no column sums of dm / dc1)
    Case("nobias", 2, True, False, 8, (64, 64, 96), ((2, 1), (2, 1)), False, 1, ((0, 1), (0,), (0, 1))),
]
BY_NAME = {c.name: c for c in CASES}
BF16_CASES = ("enc2d", "dec2d", "text1d", "textT1d")

# A/B switches, set on module attributes (pytest monkeypatch): name -> [(module, attribute, value)]
ROUTES = {
    "default": [],
    "f32fwd": [(ops, "BLOCK_FRONT_F32_FWD", True)],
    "nofront": [(ops, "BLOCK_FRONT", False)],
    "mat0": [(trunk, "MATERIALIZE", "0")],
    "nomix": [(trunk, "FUSE_MIX", False)],
    "nonext": [(trunk, "FUSE_NEXT_REDUCE", False)],
    "nolanes": [(trunk, "LANES", [])],
}
ROUTE_CASES = ("enc2d", "dec2d")
ROUTE_MODES = ("train_nodrop", "train")


def set_route(monkeypatch, route: str):
    for mod, attr, value in ROUTES[route]:
        monkeypatch.setattr(mod, attr, value)


# ---- layouts --------------------------------------------------------------------------------------------------------
def to_nhwc(t, twod: bool):
    """reference [N, C, H, W] / [N, C, L] -> the kernels' [N, H, W, C] / [N, 1, L, C]"""
    return (t.permute(0, 2, 3, 1) if twod else t.permute(0, 2, 1).unsqueeze(1)).contiguous()


# ---- builders -------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    case: Case
    seed: int
    blocks: List[trunk.BlockSpec]           # on the CPU, fp32; runs work on deep copies
    strides: List[Tuple[int, int]]          # the reference's (stride, padding) per block
    x: torch.Tensor                         # reference layout, fp32
    gout: torch.Tensor                      # upstream gradient, reference layout, fp32


def _fill(p: ResBlockParams, gen):
    """conv weights as PackedConv.reset_parameters draws them; BN affine parameters as tests/test_hip_ops_gpu.py::make_bn draws
    them, running statistics as its mode 2 does (never the (0, 1) of a fresh BatchNorm)"""
    with torch.no_grad():
        for conv in (p.conv1, p.conv2, p.short[0]):
            fan_in = (conv.cout if conv.kind == "convT" else conv.cin) * conv.weight.shape[0]
            bound = 1.0 / math.sqrt(fan_in)
            conv.weight.copy_((torch.rand(conv.weight.shape, generator=gen) * 2 - 1) * bound)
            if conv.bias is not None:
                conv.bias.copy_((torch.rand(conv.bias.shape, generator=gen) * 2 - 1) * bound)
        for bn in (p.bn1, p.bn2, p.short[1]):
            c = bn.weight.numel()
            bn.weight.copy_(1 + 0.3 * torch.randn(c, generator=gen))
            bn.bias.copy_(0.2 * torch.randn(c, generator=gen))
            bn.running_mean.copy_(0.1 * torch.randn(c, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(c, generator=gen))


def build(case: Case, seed: Optional[int] = None) -> Built:
    """the chain's BlockSpecs with the geometries mimic_amd/nets.py gives its networks, and seeded inputs"""
    seed = case.seed if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    k = (4, 4) if case.twod else (4,)
    short_name = "upsample" if case.transposed else "downsample"
    blocks, size = [], case.size
    for i, (st, pd) in enumerate(case.plan):
        ci, co = case.chans[i], case.chans[i + 1]
        p = ResBlockParams(ci, co, k, case.transposed, case.main_bias, short_name)
        _fill(p, gen)
        if case.transposed:
            so = (size - 1) * st - 2 * pd + 4
            st_eff = 4 if (st == 1 and size == 1) else st     # (a k4 s1 p0 transposed conv on one pixel is a k4 s4 p0 one)
            small, big = size, so
        else:
            so = (size + 2 * pd - 4) // st + 1
            st_eff = st
            small, big = so, size
        if case.twod:
            g1 = Geom(1, size, size, size, size, ci, ci, 1, 1, 1, 1, 0, 0, case.transposed)
            g2 = Geom(1, small, small, big, big, ci, co, 4, 4, st_eff, st_eff, pd, pd, case.transposed)
        else:
            g1 = Geom(1, 1, size, 1, size, ci, ci, 1, 1, 1, 1, 0, 0, case.transposed)
            g2 = Geom(1, 1, small, 1, big, ci, co, 1, 4, 1, st_eff, 0, pd, case.transposed)
        blocks.append(trunk.BlockSpec(p, g1, g2, case.twod, f"chain.{i}.0"))
        size = so
    sp_in = (case.size,) * (2 if case.twod else 1)
    sp_out = (size,) * (2 if case.twod else 1)
    x = torch.randn((case.batch, case.chans[0]) + sp_in, generator=gen)
    gout = torch.randn((case.batch, case.chans[-1]) + sp_out, generator=gen)
    return Built(case, seed, blocks, list(case.plan), x, gout)


def ref_state(built: Built, dtype) -> Dict[str, torch.Tensor]:
    """the blocks' parameters under the reference's key names and layouts"""
    sd = {}
    for spec in built.blocks:
        p, n = spec.params, spec.name
        convs = [("conv1", p.conv1), ("conv2", p.conv2), (f"{p.short_name}.0", p.short[0])]
        for key, conv in convs:
            sd[f"{n}.{key}.weight"] = unpack_weight(conv.weight.detach(), conv.kind, conv.k).to(dtype)
            if conv.bias is not None:
                sd[f"{n}.{key}.bias"] = conv.bias.detach().to(dtype)
        for key, bn in (("bn1", p.bn1), ("bn2", p.bn2), (f"{p.short_name}.1", p.short[1])):
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                sd[f"{n}.{key}.{leaf}"] = getattr(bn, leaf).detach().to(dtype)
    return sd


# ---- the reference ----------------------------------------------------------------------------------------------------
class _RecordRelu:
    """stands in for torch.nn.functional inside the oracle while a reference runs: F.relu's inputs are kept"""

    def __init__(self, sink):
        self._sink = sink

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, t, *a, **kw):
        self._sink.append(t.detach())
        return F.relu(t, *a, **kw)


@dataclass
class RefRun:
    tensors: Dict[str, torch.Tensor]        # 'out', 'dx', parameter gradients (packed layout), '<bn>.running_mean/var'; kernels' layouts
    relu_in: List[torch.Tensor]             # every ReLU input in call order (bn1, bn2 of block 0, bn1, bn2 of block 1), NHWC
    masks: Dict[str, torch.Tensor]


def run_reference(built: Built, mode: str, dtype, masks=None, bf16: bool = False, x=None, gout=None) -> RefRun:
    """_resblock chained under autograd in `dtype`.  mode 'train': masks drawn by the oracle (seeded) unless given."""
    case = built.case
    sd = {k: v.clone().requires_grad_(not k.split(".")[-1].startswith("running")) for k, v in ref_state(built, dtype).items()}
    x = (built.x if x is None else x).to(dtype).clone().requires_grad_(True)
    gout = (built.gout if gout is None else gout).to(dtype)
    ctx = R.Ctx(mode, masks=masks, draw_masks=masks is None, record_masks=True, mask_seed=built.seed + 1000, bf16=bf16)
    relu_in: List[torch.Tensor] = []
    saved_f = R.F
    R.F = _RecordRelu(relu_in)
    try:
        h = x
        for spec, (st, pd) in zip(built.blocks, built.strides):
            h = R._resblock(sd, spec.name, h, ctx, stride=st, pad=pd, transposed=case.transposed, twod=case.twod,
                            short_name=spec.params.short_name)
    finally:
        R.F = saved_f
    (h * gout).sum().backward()
    t = {"out": to_nhwc(h.detach(), case.twod), "dx": to_nhwc(x.grad, case.twod)}
    for spec in built.blocks:
        p = spec.params
        for key, conv in (("conv1", p.conv1), ("conv2", p.conv2), (f"{p.short_name}.0", p.short[0])):
            t[f"{spec.name}.{key}.weight"] = pack_weight(sd[f"{spec.name}.{key}.weight"].grad, conv.kind)
            if conv.bias is not None:
                t[f"{spec.name}.{key}.bias"] = sd[f"{spec.name}.{key}.bias"].grad
        for key in ("bn1", "bn2", f"{p.short_name}.1"):
            for leaf in ("weight", "bias"):
                t[f"{spec.name}.{key}.{leaf}"] = sd[f"{spec.name}.{key}.{leaf}"].grad
    for k, v in ctx.new_running.items():
        t[k] = v.detach()
    return RefRun(t, [to_nhwc(r, case.twod) for r in relu_in], dict(ctx.masks))


@dataclass
class Reference:
    built: Built
    r64: RefRun
    r32: RefRun
    margin: float                           # min |ReLU input| of the fp64 run
    dev: Dict[str, float]                   # per tensor: max |fp32 - fp64| / scale, floored at DEV_FLOOR


def scale_of(name: str, truth: Dict[str, torch.Tensor]) -> float:
    """max |truth|; a bias takes its companion weight gradient's when that is larger (tests/test_model_gpu.py::check_grads): a conv
    bias feeding a train-mode BatchNorm has an analytically zero gradient and holds only rounding noise"""
    s = truth[name].abs().max().item()
    if name.endswith(".bias") and name[:-4] + "weight" in truth:
        s = max(s, truth[name[:-4] + "weight"].abs().max().item())
    return max(s, 1e-30)


def error(name: str, got, truth: Dict[str, torch.Tensor]) -> float:
    """max over the elements of |got - truth| on the tensor's scale"""
    got = got.detach().double().cpu()
    ref = truth[name].double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    return (got - ref).abs().max().item() / scale_of(name, truth)


def make_reference(case: Case, seed: int, mode: str) -> Reference:
    built = build(case, seed)
    r64 = run_reference(built, mode, torch.float64)
    r32 = run_reference(built, mode, torch.float32, masks=r64.masks)
    assert set(r64.tensors) == set(r32.tensors)
    margin = min(r.abs().min().item() for r in r64.relu_in)
    dev = {k: max(error(k, r32.tensors[k], r64.tensors), DEV_FLOOR) for k in r64.tensors}
    return Reference(built, r64, r32, margin, dev)


@functools.lru_cache(maxsize=None)
def reference(case_name: str, mode: str) -> Reference:
    """computed once per (case, mode) and shared by every test and route; never modified"""
    return make_reference(BY_NAME[case_name], BY_NAME[case_name].seed, mode)


def assert_margin(ref: Reference):
    """from the reference alone, before anything is compared: no ReLU mask hangs on a rounding"""
    assert len(ref.r64.relu_in) == 2 * len(ref.built.blocks)
    assert ref.margin >= M, f"{ref.built.case.name}: a ReLU input of the fp64 reference lies {ref.margin:.2e} from zero (< {M})"
    worst = max(ref.dev.values())
    assert worst <= DEV_MAX, f"{ref.built.case.name}: the fp32 oracle itself strays {worst:.2e} from fp64 (> {DEV_MAX:.2e})"


@dataclass
class Bf16Reference:
    built: Built
    x: torch.Tensor                         # the inputs as stored: bf16 values
    gout: torch.Tensor
    truth: RefRun                           # plain fp64 arithmetic on the same inputs
    oracle: RefRun                          # Ctx(bf16=True) in fp64: the product's rounding points, exact sums


@functools.lru_cache(maxsize=None)
def reference_bf16(case_name: str, mode: str) -> Bf16Reference:
    built = build(BY_NAME[case_name])
    x, gout = built.x.to(BF16).float(), built.gout.to(BF16).float()
    truth = run_reference(built, mode, torch.float64, x=x, gout=gout)
    oracle = run_reference(built, mode, torch.float64, masks=truth.masks, bf16=True, x=x, gout=gout)
    return Bf16Reference(built, x, gout, truth, oracle)


# ---- the code under test ----------------------------------------------------------------------------------------------
class CheckedArena(trunk.BackwardArena):
    """a BackwardArena that counts the pieces it hands out and the ones that fell back to a fresh allocation"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pieces, self.fallbacks = 0, 0

    def take_misc(self, shape):
        t = super().take_misc(shape)
        self.pieces += 1
        if t.untyped_storage().data_ptr() != self.fbuf.untyped_storage().data_ptr():
            self.fallbacks += 1
        return t


@dataclass
class TrunkRun:
    tensors: Dict[str, torch.Tensor]        # the names of RefRun.tensors
    saved: list
    blocks: List[trunk.BlockSpec]
    arena: CheckedArena
    grads: Dict[str, torch.Tensor]
    running_before: Dict[str, torch.Tensor]


def run_trunk(built: Built, mode: str, device, masks=None, bf16: bool = False, x=None, gout=None) -> TrunkRun:
    """trunk_forward -> trunk_backward -> apply_running_updates on copies of the case's blocks, as mimic_amd/nets.py drives them
    (the stem's column statistics are made here).  bf16: activations bf16, wsel hands out the bf16 weight copies."""
    case = built.case
    device = torch.device(device)
    blocks = copy.deepcopy(built.blocks)
    for spec in blocks:
        spec.params.to(device)
    training, dropout = mode != "eval", mode == "train"
    act = BF16 if bf16 else torch.float32
    xd = to_nhwc(built.x if x is None else x, case.twod).to(device=device, dtype=act)
    gd = to_nhwc(built.gout if gout is None else gout, case.twod).to(device=device, dtype=act)
    wsel = trunk._master_weight
    if bf16:
        copies = {}
        for spec in blocks:
            for conv in (spec.params.conv1, spec.params.conv2, spec.params.short[0]):
                copies[id(conv)] = conv.weight.detach().to(BF16)
        wsel = lambda mod: copies[id(mod)]
    running_before = {}
    for spec in blocks:
        p = spec.params
        for key, bn in (("bn1", p.bn1), ("bn2", p.bn2), (f"{p.short_name}.1", p.short[1])):
            running_before[f"{spec.name}.{key}.running_mean"] = bn.running_mean.detach().clone()
            running_before[f"{spec.name}.{key}.running_var"] = bn.running_var.detach().clone()
    with torch.no_grad():
        stats = trunk.StatsArena(trunk.stats_needed(blocks), device, training)
        st0 = stats.take(case.chans[0])
        if training:
            x2 = xd.reshape(-1, case.chans[0]).double()
            st0[0].copy_(x2.sum(0))
            st0[1].copy_((x2 * x2).sum(0))
        out, saved, running = trunk.trunk_forward(blocks, xd, st0, training, dropout, trunk.MaskSource(replay=masks), stats,
                                                  case.batch, wsel)
        arena = CheckedArena(blocks, device)
        grads: Dict[str, torch.Tensor] = {}
        dx, _ = trunk.trunk_backward(blocks, saved, gd, grads, wsel, arena)
        assert len(running) == (3 * len(blocks) if training else 0)
        trunk.apply_running_updates(running)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
    t = {"out": out, "dx": dx}
    t.update(grads)
    if training:
        for spec in blocks:
            p = spec.params
            for key, bn in (("bn1", p.bn1), ("bn2", p.bn2), (f"{p.short_name}.1", p.short[1])):
                t[f"{spec.name}.{key}.running_mean"] = bn.running_mean.detach()
                t[f"{spec.name}.{key}.running_var"] = bn.running_var.detach()
    return TrunkRun(t, saved, blocks, arena, grads, running_before)


# ---- host-side invariants ---------------------------------------------------------------------------------------------
def assert_host_state(run: TrunkRun, mode: str):
    """every gradient a view into the BackwardArena, the views pairwise disjoint, no piece from a fresh allocation;
    pending_batches counted once per training forward; an eval forward leaves the running statistics alone"""
    ar = run.arena
    base = ar.fbuf.untyped_storage().data_ptr()
    lo, hi = ar.fbuf.data_ptr(), ar.fbuf.data_ptr() + ar.fbuf.numel() * 4
    assert ar.fallbacks == 0 and ar.pieces > 0, (ar.fallbacks, ar.pieces)
    spans = []
    for name, g in run.grads.items():
        assert g.dtype == torch.float32 and g.is_contiguous(), name
        assert g.untyped_storage().data_ptr() == base, f"{name} is not a view into the arena"
        a, b = g.data_ptr(), g.data_ptr() + g.numel() * 4
        assert lo <= a and b <= hi, name
        spans.append((a, b, name))
    spans.sort()
    for (a0, b0, n0), (a1, b1, n1) in zip(spans, spans[1:]):
        assert b0 <= a1, f"{n0} and {n1} overlap in the arena"
    for spec in run.blocks:
        p = spec.params
        for key, bn in (("bn1", p.bn1), ("bn2", p.bn2), (f"{p.short_name}.1", p.short[1])):
            assert bn.pending_batches == (0 if mode == "eval" else 1), (spec.name, key, bn.pending_batches)
            if mode == "eval":
                assert torch.equal(bn.running_mean, run.running_before[f"{spec.name}.{key}.running_mean"])
                assert torch.equal(bn.running_var, run.running_before[f"{spec.name}.{key}.running_var"])


def assert_relu_patterns(run: TrunkRun, ref: RefRun):
    """a2 = relu(bn2(d1)) wherever the forward wrote it: its sign pattern is the reference's, element for element"""
    seen = 0
    for i, sv in enumerate(run.saved):
        if sv.get("a2") is not None:
            seen += 1
            got = sv["a2"].detach().float().cpu() > 0
            want = ref.relu_in[2 * i + 1] > 0
            assert got.shape == want.shape
            assert torch.equal(got, want), f"block {i}: {(got != want).sum().item()} ReLU masks of bn2 differ from the reference"
    return seen


# ---- the bf16 family's gates ------------------------------------------------------------------------------------------
BF16_CAP_MAX = 0.15     # tests/g7_util.py::check_bf16_case: no rel-L2 cap of a bf16 gradient may exceed it


def bf16_figures(run: TrunkRun, ref: Bf16Reference) -> Dict[str, Tuple[float, float, float]]:
    """per tensor: (rel-L2 against the bf16-mode oracle, distance to the fp64 truth, the bf16-mode oracle's own distance to it), the
    norms of tests/g7_util.py: denominators floored at the bf16 noise floor 2e-2 scale sqrt(n) of a (near-)zero gradient"""
    fig = {}
    for name, truth in ref.truth.tensors.items():
        if name.endswith(("running_mean", "running_var")):
            continue
        got = run.tensors[name].detach().double().cpu()
        orc, truth = ref.oracle.tensors[name].double(), truth.double()
        assert got.shape == truth.shape and torch.isfinite(got).all(), name
        floor = 2e-2 * scale_of(name, ref.truth.tensors) * truth.numel() ** 0.5
        fig[name] = ((got - orc).norm().item() / max(orc.norm().item(), floor),
                     (got - truth).norm().item() / max(truth.norm().item(), floor),
                     (orc - truth).norm().item() / max(truth.norm().item(), floor))
    return fig


def assert_bf16(run: TrunkRun, ref: Bf16Reference, cap: float, tag: str):
    """rel-L2 against the bf16-mode oracle <= cap; as close to the fp64 truth as the bf16-mode oracle is (1.5 x + 2e-2)"""
    assert cap <= BF16_CAP_MAX
    fig = bf16_figures(run, ref)
    bad = {k: v for k, v in fig.items() if v[0] > cap or v[1] > 1.5 * v[2] + 2e-2}
    assert not bad, f"{tag}: (rel-L2 vs bf16 oracle, distance to fp64, the oracle's distance) {bad}"
    return fig


# ---- which route ran ----------------------------------------------------------------------------------------------------
RECORDED = ["conv_fwd", "conv_dgrad", "conv_wgrad", "block_out_fwd", "bn_relu_apply", "bn_bwd_reduce", "block_out_bwd",
            "bn_bwd_apply", "bn_running_update", "block_front_stats", "block_front_apply", "block_front_bwd"]


class Recorder:
    """wraps mimic_amd.ops.<op> (whatever is installed there: the HIP ops or their emulation) and keeps what trunk.py asked for"""

    def __init__(self, monkeypatch):
        self.calls: List[Tuple[str, dict]] = []
        for name in RECORDED:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, inner):
        def call(*a, **kw):
            info = {k: kw.get(k) is not None for k in ("mix", "bn_in", "mask", "add", "next_s", "relu_bn", "dbias")}
            info["bn_mode"] = kw["relu_bn"].mode if kw.get("relu_bn") is not None else 0
            info["stream"] = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0
            self.calls.append((name, info))
            return inner(*a, **kw)
        return call

    def count(self, name, **flags):
        return sum(1 for n, info in self.calls if n == name and all(info[k] == v for k, v in flags.items()))

    def streams(self, name):
        return {info["stream"] for n, info in self.calls if n == name}


def expected_calls(case: Case, mode: str, route: str, bf16: bool = False) -> Dict[Tuple, int]:
    """the launches a two-block chain must make, from the case table and the route's meaning alone"""
    nb = len(case.plan)
    training = mode != "eval"
    fb = set(case.fronts[MODES.index(mode)])
    if route in ("nofront", "mat0"):
        fb = set()
    ff = fb if (bf16 or route == "f32fwd") else set()
    materialize = route != "mat0"
    mixed = (case.mix or bf16) and route != "nomix"
    fuse_next = route != "nonext"
    nfb, nff = len(fb), len(ff)
    return {
        ("block_front_stats",): nff if training else 0,
        ("block_front_apply",): nff,
        ("block_front_bwd",): nfb,
        ("block_front_bwd", "dbias"): nfb if case.main_bias else 0,
        ("bn_relu_apply",): (nb - nff) if materialize else 0,
        ("conv_fwd",): 3 * nb - nff,
        ("conv_fwd", "mix"): nb if mixed else 0,
        ("conv_fwd", "bn_in"): (nb - nff) + (0 if materialize else nb),
        ("block_out_fwd",): 0 if mixed else nb,
        ("bn_bwd_reduce",): 1 if fuse_next else nb,
        ("block_out_bwd",): nb,
        ("conv_dgrad",): 3 * nb - nfb,
        ("conv_dgrad", "mode3"): nff,
        ("conv_wgrad",): 3 * nb - nfb,
        ("conv_wgrad", "bn_in"): (nb - nfb) + (0 if materialize else nb),
        ("bn_bwd_apply",): 2 * nb - nfb,
        ("bn_bwd_apply", "add"): nb,
        ("bn_bwd_apply", "next_s"): (nb - 1) if fuse_next else 0,
        ("bn_running_update",): 1 if training else 0,
    }


def recorded_calls(rec: Recorder) -> Dict[Tuple, int]:
    return {
        ("block_front_stats",): rec.count("block_front_stats"),
        ("block_front_apply",): rec.count("block_front_apply"),
        ("block_front_bwd",): rec.count("block_front_bwd"),
        ("block_front_bwd", "dbias"): rec.count("block_front_bwd", dbias=True),
        ("bn_relu_apply",): rec.count("bn_relu_apply"),
        ("conv_fwd",): rec.count("conv_fwd"),
        ("conv_fwd", "mix"): rec.count("conv_fwd", mix=True),
        ("conv_fwd", "bn_in"): rec.count("conv_fwd", bn_in=True),
        ("block_out_fwd",): rec.count("block_out_fwd"),
        ("bn_bwd_reduce",): rec.count("bn_bwd_reduce"),
        ("block_out_bwd",): rec.count("block_out_bwd"),
        ("conv_dgrad",): rec.count("conv_dgrad"),
        ("conv_dgrad", "mode3"): rec.count("conv_dgrad", bn_mode=3),
        ("conv_wgrad",): rec.count("conv_wgrad"),
        ("conv_wgrad", "bn_in"): rec.count("conv_wgrad", bn_in=True),
        ("bn_bwd_apply",): rec.count("bn_bwd_apply"),
        ("bn_bwd_apply", "add"): rec.count("bn_bwd_apply", add=True),
        ("bn_bwd_apply", "next_s"): rec.count("bn_bwd_apply", next_s=True),
        ("bn_running_update",): rec.count("bn_running_update"),
    }


def assert_route(rec: Recorder, case: Case, mode: str, route: str, bf16: bool = False):
    got, want = recorded_calls(rec), expected_calls(case, mode, route, bf16)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, f"{case.name} {mode} {route}: launches (seen, expected) {diff}"


def all_params():
    """(case, mode, route) of the fp32 family: every case in every mode by default, every switch on the two 64-channel chains"""
    out = [(c.name, m, "default") for c in CASES for m in MODES]
    out += [(c, m, r) for c in ROUTE_CASES for m in ROUTE_MODES for r in ROUTES if r != "default"]
    return out
