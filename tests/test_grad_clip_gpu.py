"""--max_grad_norm on the GPU (include/mopoe_hip_optim.h, csrc/adam.hip): the gradient-norm kernels against the fp64 norm, the
clipped Adam step against the unclipped one (bit for bit when nothing is clipped), against its restatement
(tests/torch_backend_clip.py) and under non-finite gradients -- all between the guard bands of tests/arena.py -- then the
whole model: eager against the captured hipGraph, against an unclipped run, data parallel in a child process, and two
epochs through the launcher.

Guard-band coverage of the clip header (checked by tests/test_grad_clip_cpu.py against the header and against this table,
and below against what the library was really asked for): GUARDED."""
import ctypes as C
import math
import os
import sys
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

import torch_backend_clip as TBC
from arena import Arena, CALLED_UNDER_ARENA, outputs_in

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PATHS = [REPO, os.path.join(REPO, "mopoe-mimic_amd"), os.path.join(REPO, "oracle"), HERE]

GUARDED = {
    "mopoe_grad_norm": "test_grad_norm_between_guard_bands",
    "mopoe_adam_step_clipped": "test_clipped_step_below_the_bound_is_the_unclipped_step",
}

# the record set: sizes below / at / across the 4-element vector and the 4096-element chunk, several chunks, then 130 records
# of 7 elements (three launches of 64 records), one record without a gradient, one of size 0
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 1] + [7] * 130
NO_GRAD, EMPTY, OFFSET = len(SIZES), len(SIZES) + 1, 6        # record numbers; OFFSET: its gradient starts one float off 16 bytes
N_RECORDS = len(SIZES) + 2
ULP = 2.0 ** -23         # the issue's bound: double arithmetic, ONE rounding of the result to float (2^-24), with margin 2


@pytest.fixture(scope="module")
def arena():
    # (every record is a view of its own with >= 1 MiB of guard on both sides: ~570 views for the Adam cases)
    from mimic_amd import ops
    ops.lib()      # loaded before the first outputs_in, which wraps the handle it finds to record the entry points used
    return Arena(DEV, capacity=1 << 30, capacity64=16 << 20)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8).to("cpu", copy=True)      # (a snapshot, wherever t lives)


def _sizes():
    return SIZES + [33, 0]


def _gradients(kind, seed=0):
    """CPU gradients of the record set (None for NO_GRAD).  wide: magnitudes 1e-20 .. 1e20, one element exactly 1e20 (its
    square leaves float range; the norm does not); moderate: what an Adam step in float can digest (v = g^2)"""
    gen = torch.Generator().manual_seed(100 + seed)
    out = []
    for i, n in enumerate(_sizes()):
        if i == NO_GRAD:
            out.append(None)
            continue
        g = torch.randn(n, generator=gen)
        if kind == "wide":
            g = g * 10.0 ** (torch.rand(n, generator=gen) * 40.0 - 20.0)
        else:
            g = g * (3.0 if i % 2 else 0.05)
        out.append(g.float())
    if kind == "wide":
        out[7][4097] = 1e20
        out[0][0] = 1e-20
    return out


def _norm64(grads):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads if g is not None and g.numel()))


def _need(grads):
    return TBC.grad_norm_partials([g.numel() for g in grads if g is not None])


def _place_grads(arena, grads):
    placed = []
    for i, g in enumerate(grads):
        if g is None:
            placed.append(None)
        elif g.numel() == 0:
            placed.append(torch.empty(0, device=DEV))
        else:
            placed.append(arena.place(g, 4 if i == OFFSET else 0, name=f"g{i}"))
    assert placed[OFFSET].data_ptr() % 16 == 4
    return placed


STATE0 = [7.0, 7.0, 7.0, 5.0]        # garbage in the three entries a call overwrites; five steps skipped so far


def _norm_call(arena, grads, max_norm, extra_scratch=3):
    """ops.grad_norm between guard bands -> (state, scratch, placed gradients), after the checks every call gets: guards
    untouched, nothing allocated, gradients unchanged, scratch beyond the partials unchanged"""
    from mimic_amd import ops
    arena.reset()
    placed = _place_grads(arena, grads)
    before = [None if g is None else _bits(g) for g in placed]
    state = arena.place(torch.tensor(STATE0), name="state")
    need = _need(grads)
    scratch = arena.place(torch.full((need + extra_scratch,), 123.0, dtype=torch.float64), name="scratch")
    CALLED_UNDER_ARENA.clear()
    with outputs_in(arena) as px:
        ops.grad_norm(placed, max_norm, state, scratch)
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert not px.allocated and "mopoe_grad_norm" in CALLED_UNDER_ARENA
    for g, b in zip(placed, before):
        assert g is None or torch.equal(_bits(g), b), "a gradient was modified"
    assert bool((scratch[need:] == 123.0).all()), "scratch beyond the partials was written"
    return state, scratch, placed


# ---- the norm kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["wide", "moderate"])
def test_grad_norm_between_guard_bands(arena, kind):
    grads = _gradients(kind)
    ref = _norm64(grads)
    assert math.isfinite(ref) and (kind != "wide" or ref >= 1e20)
    for max_norm in (2.0 * ref, ref / 3.0):
        state, scratch, _ = _norm_call(arena, grads, max_norm)
        norm, scale, skip, total = (float(x) for x in state.double().cpu())
        want_scale = min(1.0, max_norm / (ref + 1e-6))
        print(f"grad_norm[{kind}] norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.3e}; scale {scale!r} want {want_scale!r}")
        assert abs(norm - ref) <= ULP * ref, (norm, ref)
        assert abs(scale - want_scale) <= ULP * want_scale, (scale, want_scale)
        assert (scale == 1.0) == (max_norm > ref) and skip == 0.0 and total == STATE0[3]
        # deterministic: a second call leaves the same bits in the state and in every partial
        bits = (_bits(state), _bits(scratch))
        state2, scratch2, _ = _norm_call(arena, grads, max_norm)
        assert torch.equal(_bits(state2), bits[0]) and torch.equal(_bits(scratch2), bits[1])


def test_grad_norm_of_single_records_and_of_nothing(arena):
    """every size of the set alone, aligned and one float off; no gradient at all: norm 0, scale 1"""
    gen = torch.Generator().manual_seed(7)
    from mimic_amd import ops
    for n in sorted(set(SIZES)):
        g = torch.randn(n, generator=gen)
        ref = float(g.double().pow(2).sum().sqrt())
        for off in (0, 4):
            arena.reset()
            gp = arena.place(g, off, name="g")
            state = arena.place(torch.tensor(STATE0), name="state")
            scratch = arena.place(torch.zeros((n + 4095) // 4096, dtype=torch.float64), name="scratch")
            with outputs_in(arena):
                ops.grad_norm([gp], 1e30, state, scratch)
            torch.cuda.synchronize()
            arena.assert_untouched()
            assert abs(float(state[0]) - ref) <= ULP * ref, (n, off, float(state[0]), ref)
            assert float(state[1]) == 1.0 and float(state[2]) == 0.0
    arena.reset()
    state = arena.place(torch.tensor(STATE0), name="state")
    scratch = arena.place(torch.full((1,), 123.0, dtype=torch.float64), name="scratch")
    with outputs_in(arena):
        ops.grad_norm([None, torch.empty(0, device=DEV)], 1.0, state, scratch)
        ops.grad_norm([], 1.0, state, scratch)
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert state.cpu().tolist() == [0.0, 1.0, 0.0, 5.0] and float(scratch[0]) == 123.0


def _raw_records(grads):
    from mimic_amd import ops
    arr = (ops._AdamSeg * len(grads))()
    for i, g in enumerate(grads):
        arr[i] = ops._AdamSeg(None, g.data_ptr(), None, None, None, g.numel())
    return arr


def test_grad_norm_refuses_what_it_cannot_run(arena):
    from mimic_amd import ops
    grads = _gradients("moderate")
    arena.reset()
    placed = _place_grads(arena, grads)
    state = arena.place(torch.tensor(STATE0), name="state")
    need = _need(grads)
    small = arena.place(torch.full((need - 1,), 123.0, dtype=torch.float64), name="scratch")
    with outputs_in(arena):
        with pytest.raises(ops.MopoeHipError, match="scratch"):
            ops.grad_norm(placed, 1.0, state, small)
        for bad in (-1.0, float("nan"), float("inf")):
            big = small      # (refused on max_norm before the size is looked at)
            with pytest.raises(ops.MopoeHipError, match="max_norm"):
                ops.grad_norm(placed[:3], bad, state, big)
        # a NULL state / scratch pointer: only the C ABI can be handed one
        arr = _raw_records(placed[:3])
        lib = ops.lib()
        for st_ptr, sc_ptr in ((None, C.c_void_p(small.data_ptr())), (C.c_void_p(state.data_ptr()), None)):
            rc = lib.mopoe_grad_norm(arr, 3, C.c_double(1.0), sc_ptr, C.c_int64(small.numel()), st_ptr, ops._stream())
            with pytest.raises(ops.MopoeHipError, match="NULL"):
                ops._check(rc)
        p = placed[0]
        one = (ops._AdamSeg * 1)(ops._AdamSeg(p.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), None, 1))
        rc = lib.mopoe_adam_step_clipped(one, 1, None, None, C.c_double(1e-3), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8),
                                         C.c_void_p(state.data_ptr()), None, ops._stream())
        with pytest.raises(ops.MopoeHipError, match="NULL"):
            ops._check(rc)
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert state.cpu().tolist() == STATE0 and bool((small == 123.0).all())
    for g, c in zip(placed, grads):
        assert g is None or torch.equal(g.cpu(), c)


# ---- the clipped Adam step ---------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 2e-3, 0.9, 0.999, 1e-8
WITH_P16 = (6, 7, 9)     # records that also keep a bf16 copy: 4097 (gradient off 16 bytes: scalar path), 3 * 4096 + 1, 7


def _adam_inputs(seed=1):
    gen = torch.Generator().manual_seed(seed)
    sizes = _sizes()
    return dict(p=[torch.randn(n, generator=gen) for n in sizes], m=[0.1 * torch.randn(n, generator=gen) for n in sizes],
                v=[0.1 * torch.rand(n, generator=gen) for n in sizes],
                p16=[torch.zeros(n, dtype=BF) if i in WITH_P16 else None for i, n in enumerate(sizes)],
                step=torch.tensor(2.0), coef=torch.tensor([0.25, 0.5]))


def _place_adam(arena, h, grads):
    """-> dict of placed tensors (lists keep None entries; size-0 records live outside the arena)"""
    put = lambda t, name, off=0: t if t is None else (torch.empty(0, dtype=t.dtype, device=DEV) if t.numel() == 0 else arena.place(t, off, name=name))
    d = {k: [put(t, f"{k}{i}") for i, t in enumerate(h[k])] for k in ("p", "m", "v", "p16")}
    d["g"] = _place_grads(arena, grads)
    d["step"], d["coef"] = arena.place(h["step"], name="step"), arena.place(h["coef"], name="coef")
    d["state"] = arena.place(torch.tensor(STATE0), name="state")
    d["scratch"] = arena.place(torch.full((_need(grads),), 123.0, dtype=torch.float64), name="scratch")
    return d


def _outputs(d):
    """every tensor a step may write, flattened: name -> tensor"""
    out = {}
    for k, label in (("p", "p"), ("m", "m"), ("v", "v"), ("p16", "lowp")):
        out.update({f"{label}{i}": t for i, t in enumerate(d[k]) if t is not None and t.numel()})
    out["step"], out["coef"] = d["step"], d["coef"]
    return out


def _clipped_step(arena, d, max_norm):
    from mimic_amd import ops
    before_g = [None if g is None else _bits(g) for g in d["g"]]
    CALLED_UNDER_ARENA.clear()
    with outputs_in(arena) as px:
        ops.grad_norm(d["g"], max_norm, d["state"], d["scratch"])
        ops.adam_step(d["p"], d["g"], d["m"], d["v"], d["step"], LR, B1, B2, EPS, d["coef"], lowp=d["p16"], clip=d["state"])
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert not px.allocated and {"mopoe_grad_norm", "mopoe_adam_step_clipped"} <= CALLED_UNDER_ARENA
    assert "mopoe_adam_step" not in CALLED_UNDER_ARENA
    for g, b in zip(d["g"], before_g):
        assert g is None or torch.equal(_bits(g), b), "a gradient was rewritten"


def _close(name, got, ref, rtol, atol_rel):
    """the bar of tests/test_hip_ops_gpu.py: check"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs()
    bound = atol_rel * scale + rtol * ref.abs()
    assert bool(torch.isfinite(got).all()), name
    assert bool((err <= bound).all()), (name, err.max().item(), scale)


def test_clipped_step_below_the_bound_is_the_unclipped_step(arena):
    """norm below max_norm: scale is exactly 1 and every output equals, bit for bit, ops.adam_step on copies"""
    from mimic_amd import ops
    grads, h = _gradients("moderate"), _adam_inputs()
    arena.reset()
    d = _place_adam(arena, h, grads)
    twin = {k: [None if t is None else t.clone() for t in d[k]] for k in ("p", "m", "v", "p16")}
    twin.update(step=d["step"].clone(), coef=d["coef"].clone(), g=d["g"])
    ops.adam_step(twin["p"], twin["g"], twin["m"], twin["v"], twin["step"], LR, B1, B2, EPS, twin["coef"], lowp=twin["p16"])
    _clipped_step(arena, d, 2.0 * _norm64(grads))
    assert d["state"].cpu().tolist()[1:] == [1.0, 0.0, 5.0]
    got, want = _outputs(d), _outputs(twin)
    assert set(got) == set(want) and float(d["step"]) == 3.0
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    # the records without a gradient kept their values
    for k in ("p", "m", "v"):
        assert torch.equal(d[k][NO_GRAD].cpu(), h[k][NO_GRAD])


def test_clipped_step_above_the_bound_against_the_restatement(arena):
    """norm above max_norm: against tests/torch_backend_clip.py with the bars tests/test_guarded_ops_gpu.py: test_adam_step
    uses against its restatement, (2e-6, 2e-7): the one added operation is a float multiply"""
    grads, h = _gradients("moderate"), _adam_inputs()
    arena.reset()
    d = _place_adam(arena, h, grads)
    max_norm = _norm64(grads) / 3.0
    _clipped_step(arena, d, max_norm)
    ref = {k: [None if t is None else t.clone() for t in h[k]] for k in ("p", "m", "v", "p16")}
    ref.update(step=h["step"].clone(), coef=h["coef"].clone())
    state = torch.tensor(STATE0)
    TBC.grad_norm(grads, max_norm, state, torch.zeros(_need(grads), dtype=torch.float64))
    TBC.adam_step(ref["p"], grads, ref["m"], ref["v"], ref["step"], LR, B1, B2, EPS, None, lowp=ref["p16"], clip=state)
    assert 0.3 < float(state[1]) < 0.34 and abs(float(d["state"][1]) - float(state[1])) <= ULP * float(state[1])
    got, want = _outputs(d), _outputs(ref)
    for k in got:
        if k == "coef":
            continue                      # (the restatement keeps its coefficients on the host)
        if k.startswith("lowp"):
            assert torch.equal(got[k].cpu(), got["p" + k[4:]].cpu().to(BF)), k       # the updated parameter rounded once
        else:
            _close(k, got[k].reshape(-1), want[k].reshape(-1), 2e-6, 2e-7)
    assert float(d["step"]) == 3.0
    # ... and the scale reached the moments: they differ from an unclipped step's by far more than the bar
    plain = [t.clone() for t in h["m"]]
    assert float((d["m"][7].cpu() - (B1 * plain[7] + (1 - B1) * grads[7])).abs().max()) > 1e-3


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step_on_the_device(arena, bad):
    """one element inf / nan: every output keeps its bits, skip = 1, skipped_total += 1 per call; the next finite call is step 3"""
    grads, h = _gradients("moderate"), _adam_inputs()
    arena.reset()
    d = _place_adam(arena, h, grads)
    before = {k: _bits(t) for k, t in _outputs(d).items()}
    where = d["g"][7]
    good = float(where[4100])
    where[4100] = bad
    for k in (1, 2):
        _clipped_step(arena, d, 1.0)
        for name, t in _outputs(d).items():
            assert torch.equal(_bits(t), before[name]), (name, k)
        norm, scale, skip, total = d["state"].cpu().tolist()
        assert not math.isfinite(norm) and scale == 0.0 and skip == 1.0 and total == STATE0[3] + k
    where[4100] = good
    _clipped_step(arena, d, 1.0)
    norm, scale, skip, total = d["state"].cpu().tolist()
    assert math.isfinite(norm) and 0.0 < scale < 1.0 and skip == 0.0 and total == STATE0[3] + 2
    assert float(d["step"]) == 3.0
    out = _outputs(d)
    for name, t in out.items():
        assert bool(torch.isfinite(t.float()).all()), name
        if name[0] in "pmv" and int(name[1:]) != NO_GRAD:
            assert not torch.equal(_bits(t), before[name]), name


# ---- the whole model -----------------------------------------------------------------------------------------------------------------
MODEL_LR, N_STEPS = 1e-3, 5        # two set-up steps on batch 0 + three steps, as tests/test_model_gpu.py runs eager against graph


def _model_runs(kinds, max_norm=None):
    """the g0_s64 fixture's tiny model in train_nodrop, 5 steps (batch 0 twice, then batches 1..3) per kind:
    unclipped | eager | graph | eager_dp | graph_dp (the last two need an initialised process group).
    max_norm None: half of the unclipped first step's norm.  -> {kind: {...}}, max_norm"""
    import mopoe_ref as R
    from golden_util import cfg_from, g0_state, load
    from model_util import build_exp
    from mimic_amd import nets, run_epochs as RE
    from mimic_amd.optim import HipAdam
    g = load("g0_s64")
    cfg = cfg_from(g["cfg"])
    batches = [R.synthetic_batch(cfg, cfg.batch_size, seed=10 + i) for i in range(4)]
    eps = batches[0][1]
    dev = lambda b: ({k: v.cuda() for k, v in b[0].items()}, None)
    out = {}
    for kind in kinds:
        exp = build_exp(cfg, g0_state(g), "cuda", "train_nodrop", eps=eps)
        exp.flags.initial_learning_rate = MODEL_LR
        exp.flags.max_grad_norm = 1e30 if kind == "unclipped" else max_norm      # (1e30: the norm is reported, nothing is clipped)
        reducer = None
        if kind.endswith("_dp"):
            from mimic_amd.parallel import GradAllReducer
            reducer = GradAllReducer(exp.mm_vae, 1, force=True)
            assert reducer.active
            reducer.broadcast_parameters()
        exp.set_optimizer()
        opt = exp.optimizer
        assert isinstance(opt, HipAdam) and opt.clip_state is not None
        armed = []
        real_step = opt.step
        opt.step = lambda: (armed.append(nets.EARLY_STEP[0]), real_step())[1]
        opt.early_step = lambda *a, **k: armed.append("early_step")
        pack = RE.ScalarPack(exp.flags.device)
        scalars, first_norm = [], None
        if not kind.startswith("graph"):
            for n, i in enumerate((0, 0, 1, 2, 3)):
                RE.train_step(exp, dev(batches[i]), reducer, pack)
                scalars.append(pack.read())
                if n == 0:     # (the pack's norm of the first step, and the fp64 norm of the gradients that step left in p.grad)
                    first_norm = (scalars[0]["grad_norm"], math.sqrt(sum(float(p.grad.double().pow(2).sum())
                                                                         for p in exp.mm_vae.parameters() if p.grad is not None)))
            scalars = scalars[2:]
        else:
            step = RE.GraphedTrainStep(exp, dev(batches[0]), pack, reducer, warmup=2)
            assert (step.graph_opt is not None) == (reducer is not None)
            for i in (1, 2, 3):
                step(dev(batches[i]))
                scalars.append(pack.read())
        torch.cuda.synchronize()
        out[kind] = {"scalars": scalars, "first_norm": first_norm,
                     "params": {n: p.detach().cpu().clone() for n, p in exp.mm_vae.named_parameters()},
                     "m": opt._moments[0].cpu().clone(), "armed": armed, "step": float(opt._step)}
        if reducer is not None:
            reducer.detach()
        if kind == "unclipped" and max_norm is None:
            max_norm = 0.5 * first_norm[1]
    return out, max_norm


@pytest.fixture(scope="module")
def model_runs():
    return _model_runs(("unclipped", "eager", "graph"))


def test_model_eager_and_captured_trajectories_agree(model_runs):
    """tolerances of tests/test_model_gpu.py: test_graphed_train_step_matches_eager -- losses 2e-4 relative, parameters
    within Adam's step bound 2 x 5 steps x lr"""
    runs, max_norm = model_runs
    e, g = runs["eager"], runs["graph"]
    assert len(e["scalars"]) == len(g["scalars"]) == 3 and e["step"] == g["step"] == N_STEPS
    for a, b in zip(e["scalars"], g["scalars"]):
        assert list(a)[-2:] == list(b)[-2:] == ["grad_norm", "skipped_steps"] and len(a) == len(b) == 20
        assert math.isfinite(a["total_loss"]) and abs(a["total_loss"] - b["total_loss"]) <= 2e-4 * abs(a["total_loss"]), (a, b)
        assert abs(a["grad_norm"] - b["grad_norm"]) <= 2e-4 * abs(a["grad_norm"]) and a["skipped_steps"] == b["skipped_steps"] == 0.0
    for n, p in e["params"].items():
        assert float((p - g["params"][n]).abs().max()) <= 2 * N_STEPS * MODEL_LR + 1e-6, n


def test_model_clipping_is_active_and_reports_the_norm(model_runs):
    runs, max_norm = model_runs
    u, e = runs["unclipped"], runs["eager"]
    # the norm the pack reports for the first step against the fp64 norm of p.grad on the host
    for run in (u, e):
        got, host = run["first_norm"]
        print(f"grad_norm of step 1: device {got!r} host fp64 {host!r} rel {abs(got - host) / host:.3e}")
        assert abs(got - host) <= ULP * host, (got, host)
    assert abs(max_norm - 0.5 * u["first_norm"][1]) <= 1e-12 * max_norm
    # the same first gradients, halved: first moments of step 1 onwards differ, and so do the parameters
    assert any(not torch.equal(p, e["params"][n]) for n, p in u["params"].items())
    assert float((u["m"] - e["m"]).abs().max()) > 1e-3 * float(u["m"].abs().max())
    assert all(s["skipped_steps"] == 0.0 for s in u["scalars"] + e["scalars"])


def test_model_early_updates_stay_off(model_runs):
    """nets.EARLY_STEP[0] is None whenever the optimiser steps (eager, and while the graph is captured), early_step is never called"""
    from mimic_amd import nets
    runs, _ = model_runs
    for kind in ("unclipped", "eager", "graph"):
        armed = runs[kind]["armed"]
        assert armed and all(a is None for a in armed), (kind, armed)
    assert len(runs["eager"]["armed"]) == N_STEPS and nets.EARLY_STEP[0] is None


def _dp_worker(rank, outdir, max_norm):
    for p in PATHS:
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{os.path.join(outdir, 'rdzv')}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    runs, _ = _model_runs(("eager_dp", "graph_dp"), max_norm)
    torch.save(runs, os.path.join(outdir, "out.pt"))
    dist.destroy_process_group()


def test_model_data_parallel_clips_the_reduced_gradients(model_runs):
    """the data-parallel code path with one rank over RCCL (GradAllReducer(force=True): what MOPOE_FORCE_DP=1 makes bench.py run), eager and as three
    graphs with the clip inside the optimiser graph: the same three steps as without it, to the tolerance of
    tests/test_dp_rccl_gpu.py (losses 2e-4 relative; parameters inside Adam's step bound, their median difference <= 1e-4).
    The child process runs the two data-parallel forms under the bound this process derived; the plain run is this process's"""
    plain, max_norm = model_runs
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(d, max_norm), nprocs=1, join=True)
        runs = torch.load(os.path.join(d, "out.pt"))
    ref = plain["eager"]
    for kind in ("eager_dp", "graph_dp"):
        r = runs[kind]
        assert r["step"] == N_STEPS and all(a is None for a in r["armed"])
        for a, b in zip(ref["scalars"], r["scalars"]):
            assert abs(a["total_loss"] - b["total_loss"]) <= 2e-4 * abs(a["total_loss"]), (kind, a, b)
            assert abs(a["grad_norm"] - b["grad_norm"]) <= 2e-4 * abs(a["grad_norm"]), (kind, a, b)
            assert b["skipped_steps"] == 0.0
        worst = []
        for n, p in ref["params"].items():
            diff = (p - r["params"][n]).abs()
            assert float(diff.max()) <= 2 * N_STEPS * MODEL_LR + 1e-6, (kind, n, float(diff.max()))
            worst.append(float(diff.median()))
        assert sorted(worst)[len(worst) // 2] <= 1e-4, (kind, sorted(worst)[-5:])


# ---- the launcher --------------------------------------------------------------------------------------------------------------------
def test_two_clipped_epochs_on_tensor_files_through_the_launcher(tmp_path):
    """tests/test_launcher_gpu.py: test_two_epochs_on_tensor_files_through_the_launcher with --max_grad_norm 1.0"""
    from golden_util import make_mimic_files
    from mimic_amd import main_mimic as MM
    data = tmp_path / "data"
    make_mimic_files(str(data), img_size=64, n_train=100, n_eval=30, seed=5)
    run_dir = tmp_path / "run"
    flags = MM.parse_flags(["--dataset", "mimic", "--dir_data", str(data), "--img_size", "64", "--class_dim", "32",
                            "--DIM_img", "64", "--DIM_text", "32", "--batch_size", "8", "--len_sequence", "128",
                            "--end_epoch", "2", "--initial_learning_rate", "1e-5", "--max_grad_norm", "1.0",
                            "--dir_experiment_run", str(run_dir)])
    assert flags.max_grad_norm == 1.0
    m = MM.Main(flags)
    m.setup_distributed = lambda: (setattr(m.flags, "world_size", 1), setattr(m.flags, "distributed", False))
    assert m.main() is True and m.current_tries == 0
    hist = m.history
    n_train = hist[0]["train"]["steps"]
    assert n_train >= 8 and [h["epoch"] for h in hist] == [0, 1]
    assert hist[1]["train"]["graphed_steps"] >= n_train - 1          # the clipped step is still the captured one
    for h in hist:
        last = h["train"]["last"]
        assert all(v == v and abs(v) < 1e9 for v in last.values()) and "total_loss" in h["test"]
        assert math.isfinite(last["grad_norm"]) and last["grad_norm"] > 0 and last["skipped_steps"] == 0.0
    line = MM.result_line(hist)
    assert math.isfinite(line["last_grad_norm"]) and line["last_grad_norm"] == hist[-1]["train"]["last"]["grad_norm"]
    assert line["skipped_steps"] == 0
