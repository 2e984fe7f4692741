"""--ema_decay on the GPU (include/mopoe_hip_ema.h, csrc/ema.hip): the update kernel against the fp64 recurrence under a
derived bound, the skip state, the in-place swap (bits preserved, bf16 copies rewritten), hostile values and refusals -- all
between the guard bands of tests/arena.py -- then the whole model: the average after eager and captured steps (early
per-network updates armed, off, and under --max_grad_norm), data parallel in a child process, evaluation and the checkpoint
under the averaged weights in fp32 and bf16, and two epochs through the launcher.

The bound of the update (BOUND): p - ema rounds once (2^-24 relative), the fma rounds once (2^-24 of the result), one more
2^-24 |p - ema| covers a last-bit difference in w; the recurrence is a contraction (0 < w <= 1), so the errors of earlier
steps do not grow: after T updates |ema - ref| <= 4 T 2^-24 M, M the largest |p| or |ema| the element has seen.

Guard-band coverage of the EMA header (checked by tests/test_ema_cpu.py against the header and against this table, and
below against what the library was really asked for): GUARDED."""
import copy
import ctypes as C
import math
import os
import sys
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

import torch_backend_ema as TBE
from arena import Arena, CALLED_UNDER_ARENA, outputs_in

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PATHS = [REPO, os.path.join(REPO, "mopoe-mimic_amd"), os.path.join(REPO, "oracle"), HERE]

GUARDED = {
    "mopoe_ema_update": "test_update_against_the_fp64_recurrence",
    "mopoe_ema_swap": "test_swap_exchanges_bits_and_rewrites_the_bf16_copies",
}

# the record set: sizes below / at / across the 4-element vector and the 4096-element chunk, several chunks, then 130 records
# of 7 elements (three launches of 64 records), one record of size 0
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 1] + [7] * 130
EMPTY = len(SIZES)
OFFSET = 6               # this record's p and ema start one float off 16 bytes, its p16 one element off: the scalar path
WITH_P16 = (4, 6, 7, 9)  # records that also keep a bf16 copy: 4095, 4097 (off alignment), 3 * 4096 + 1, 7
EPS24 = 2.0 ** -24


def BOUND(T, M):
    return 4 * T * EPS24 * M


@pytest.fixture(scope="module")
def arena():
    # (every record is a view of its own with >= 1 MiB of guard on both sides: ~330 views)
    from mimic_amd import ops
    ops.lib()      # loaded before the first outputs_in, which wraps the handle it finds to record the entry points used
    return Arena(DEV, capacity=1 << 30, capacity64=16 << 20)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8).to("cpu", copy=True)      # (a snapshot, wherever t lives)


def _sizes():
    return SIZES + [0]


def _draw(gen, n, i):
    """N(0, 1) with some exact zeros; record 7 carries one element of 1e20"""
    x = torch.randn(n, generator=gen)
    if n:
        x[torch.rand(n, generator=gen) < 0.05] = 0.0
    if i == 7:
        x[4097] = 1e20
    return x


def _host_set(seed=0):
    gen = torch.Generator().manual_seed(200 + seed)
    sizes = _sizes()
    p = [_draw(gen, n, i) for i, n in enumerate(sizes)]
    ema = [torch.randn(n, generator=gen) for n in sizes]
    p16 = [p[i].to(BF) if i in WITH_P16 else None for i in range(len(sizes))]
    return dict(p=p, ema=ema, p16=p16), gen


def _place(arena, h):
    """-> dict of placed tensors (lists keep None entries; the size-0 record lives outside the arena)"""
    arena.reset()
    d = {}
    for k in ("p", "ema", "p16"):
        d[k] = []
        for i, t in enumerate(h[k]):
            if t is None:
                d[k].append(None)
            elif t.numel() == 0:
                d[k].append(torch.empty(0, dtype=t.dtype, device=DEV))
            else:
                off = 0 if i != OFFSET else (2 if k == "p16" else 4)
                d[k].append(arena.place(t, off, name=f"{k}{i}"))
    assert d["p"][OFFSET].data_ptr() % 16 == 4 and d["ema"][OFFSET].data_ptr() % 16 == 4 and d["p16"][OFFSET].data_ptr() % 16 == 2
    d["step"] = arena.place(torch.tensor(1.0), name="step")
    d["clip"] = arena.place(torch.tensor([7.0, 7.0, 0.0, 5.0]), name="clip")
    return d


def _all(d):
    out = {}
    for k in ("p", "ema", "p16"):
        out.update({f"{k}:{i}": t for i, t in enumerate(d[k]) if t is not None and t.numel()})
    out["step"], out["clip"] = d["step"], d["clip"]
    return out


def _snapshot(d):
    return {k: _bits(t) for k, t in _all(d).items()}


def _same(d, snap):
    for k, t in _all(d).items():
        assert torch.equal(_bits(t), snap[k]), k


def _update(arena, d, decay, clip=None):
    from mimic_amd import ops
    CALLED_UNDER_ARENA.clear()
    with outputs_in(arena) as px:
        ops.ema_update(d["p"], d["ema"], decay, d["step"], clip=clip)
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert not px.allocated and "mopoe_ema_update" in CALLED_UNDER_ARENA


def _swap(arena, d, with_p16=True):
    from mimic_amd import ops
    CALLED_UNDER_ARENA.clear()
    with outputs_in(arena) as px:
        ops.ema_swap(d["p"], d["ema"], lowp=d["p16"] if with_p16 else None)
    torch.cuda.synchronize()
    arena.assert_untouched()
    assert not px.allocated and "mopoe_ema_swap" in CALLED_UNDER_ARENA


# ---- 1. update against fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay,steps", [(0.999, (1, 2, 89, 90, 10 ** 4, 10 ** 6)), (0.5, (1, 2, 89))])
def test_update_against_the_fp64_recurrence(arena, decay, steps):
    h, gen = _host_set()
    d = _place(arena, h)
    ref = [e.double() for e in h["ema"]]
    big = [torch.maximum(e.abs(), p.abs()).double() for e, p in zip(h["ema"], h["p"])]
    p_now = h["p"]
    other = _snapshot(d)
    for k, s in enumerate(steps):
        if k:
            p_now = [_draw(gen, n, i) for i, n in enumerate(_sizes())]
            for t, x in zip(d["p"], p_now):
                t.copy_(x)
        d["step"].fill_(float(s))
        p_bits = [_bits(t) for t in d["p"]]
        _update(arena, d, decay)
        w = TBE.weight_at(decay, s)
        ref = [r + w * (p.double() - r) for r, p in zip(ref, p_now)]
        got = [e.cpu() for e in d["ema"]]
        big = [torch.maximum(b, torch.maximum(p.abs().double(), torch.maximum(r.abs(), g.abs().double())))
               for b, p, r, g in zip(big, p_now, ref, got)]
        for t, b in zip(d["p"], p_bits):
            assert torch.equal(_bits(t), b), "p was written"
    T = len(steps)
    worst = 0.0
    for i, (g, r, b) in enumerate(zip(got, ref, big)):
        if not g.numel():
            continue
        assert bool(torch.isfinite(g).all()), i
        err = (g.double() - r).abs()
        worst = max(worst, float((err / BOUND(T, b).clamp_min(1e-300)).max()))
        assert bool((err <= BOUND(T, b)).all()), (i, float(err.max()))
    print(f"ema_update decay {decay}: worst |ema - ref| / bound = {worst:.3f} after {T} updates")
    assert abs(float(d["ema"][7][4097]) - float(ref[7][4097])) <= BOUND(T, 1e20) and float(d["ema"][7][4097]) > 1e16
    # the bf16 copies, the step counter and the clip state are not the update's to write
    for k, t in _all(d).items():
        if k.startswith(("p16:", "clip")):
            assert torch.equal(_bits(t), other[k]), k
    assert float(d["step"]) == float(steps[-1])
    # the restatement agrees to within the last-bit allowance of one update
    h2, _ = _host_set(1)
    d2 = _place(arena, h2)
    d2["step"].fill_(89.0)
    _update(arena, d2, decay)
    twin = [e.clone() for e in h2["ema"]]
    TBE.ema_update(h2["p"], twin, decay, torch.tensor(89.0))
    for i, (g, t, p) in enumerate(zip(d2["ema"], twin, h2["p"])):
        if g.numel():
            m = torch.maximum(torch.maximum(p.abs(), t.abs()), h2["ema"][i].abs()).double()
            assert bool(((g.cpu().double() - t.double()).abs() <= BOUND(1, m)).all()), i


# ---- 2. skip --------------------------------------------------------------------------------------------------------------
def test_a_skip_state_withholds_every_store(arena):
    h, _ = _host_set(2)
    d = _place(arena, h)
    d["step"].fill_(3.0)
    d["clip"].copy_(torch.tensor([float("nan"), 0.0, 1.0, 6.0]))
    snap = _snapshot(d)
    _update(arena, d, 0.9, clip=d["clip"])
    _same(d, snap)
    # skip 0: bit for bit the call without a clip state
    d["clip"].copy_(torch.tensor([3.0, 0.25, 0.0, 6.0]))
    _update(arena, d, 0.9, clip=d["clip"])
    with_clip = [_bits(e) for e in d["ema"]]
    assert any(not torch.equal(b, snap[f"ema:{i}"]) for i, b in enumerate(with_clip) if b.numel())
    d = _place(arena, h)
    d["step"].fill_(3.0)
    _update(arena, d, 0.9)
    for a, e in zip(with_clip, d["ema"]):
        assert torch.equal(a, _bits(e))


# ---- 3. swap ----------------------------------------------------------------------------------------------------------------
def test_swap_exchanges_bits_and_rewrites_the_bf16_copies(arena):
    h, _ = _host_set(3)
    d = _place(arena, h)
    snap = _snapshot(d)
    _swap(arena, d)
    for i in range(len(_sizes())):
        if not d["p"][i].numel():
            continue
        assert torch.equal(_bits(d["p"][i]), snap[f"ema:{i}"]) and torch.equal(_bits(d["ema"][i]), snap[f"p:{i}"]), i
        if d["p16"][i] is not None:
            assert torch.equal(_bits(d["p16"][i]), _bits(d["p"][i].to(BF))), i        # the new p, rounded as torch rounds
            assert not torch.equal(_bits(d["p16"][i]), snap[f"p16:{i}"])
    assert torch.equal(_bits(d["step"]), snap["step"]) and torch.equal(_bits(d["clip"]), snap["clip"])
    _swap(arena, d)
    _same(d, snap)
    # records without a bf16 copy are exchanged as well: the same set with every p16 NULL
    _swap(arena, d, with_p16=False)
    for i in range(len(_sizes())):
        if d["p"][i].numel():
            assert torch.equal(_bits(d["p"][i]), snap[f"ema:{i}"]) and torch.equal(_bits(d["ema"][i]), snap[f"p:{i}"]), i
        if d["p16"][i] is not None and d["p16"][i].numel():
            assert torch.equal(_bits(d["p16"][i]), snap[f"p16:{i}"]), i
    _swap(arena, d, with_p16=False)
    _same(d, snap)


def test_every_size_alone_aligned_and_off(arena):
    """each size of the set as the only record, aligned and one float off: update within the bound, swap exact"""
    from mimic_amd import ops
    gen = torch.Generator().manual_seed(9)
    for n in sorted(set(SIZES)):
        p, e = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        for off in (0, 4):
            arena.reset()
            pp, ee = arena.place(p, off, name="p"), arena.place(e, off, name="ema")
            lp = arena.place(p.to(BF), off // 2, name="p16")
            step = arena.place(torch.tensor(4.0), name="step")
            with outputs_in(arena):
                ops.ema_update([pp], [ee], 0.25, step)
            torch.cuda.synchronize()
            arena.assert_untouched()
            ref = e.double() + TBE.weight_at(0.25, 4) * (p.double() - e.double())
            m = torch.maximum(torch.maximum(p.abs(), e.abs()).double(), ref.abs())
            assert bool(((ee.cpu().double() - ref).abs() <= BOUND(1, m)).all()), (n, off)
            assert torch.equal(pp.cpu(), p)
            avg = ee.cpu()
            with outputs_in(arena):
                ops.ema_swap([pp], [ee], lowp=[lp])
            torch.cuda.synchronize()
            arena.assert_untouched()
            assert torch.equal(_bits(pp), _bits(avg)) and torch.equal(_bits(ee), _bits(p)) and torch.equal(_bits(lp), _bits(avg.to(BF)))


# ---- 4. hostile values -----------------------------------------------------------------------------------------------------
HOSTILE = [float("nan"), float("inf"), float("-inf"), 1e-45, -1e-40]     # the last two: denormals


def test_hostile_values_stay_where_they_are(arena):
    h, _ = _host_set(4)
    where = {"p": {}, "ema": {}}
    for j, (i, pos) in enumerate([(7, 0), (7, 4096), (7, 3 * 4096), (5, 4095), (6, 4096), (3, 4), (0, 0), (9, 3), (137, 6)]):
        key = "p" if j % 2 == 0 else "ema"
        h[key][i][pos] = HOSTILE[j % len(HOSTILE)]
        where[key].setdefault(i, []).append(pos)
    h["p16"] = [None if t is None else h["p"][i].to(BF) for i, t in enumerate(h["p16"])]
    d = _place(arena, h)
    d["step"].fill_(5.0)
    snap = _snapshot(d)
    # swap carries every word unchanged, NaN payloads and denormals included; twice is the identity on p and ema
    _swap(arena, d, with_p16=False)
    for i in range(len(_sizes())):
        if d["p"][i].numel():
            assert torch.equal(_bits(d["p"][i]), snap[f"ema:{i}"]) and torch.equal(_bits(d["ema"][i]), snap[f"p:{i}"]), i
    _swap(arena, d, with_p16=False)
    _same(d, snap)
    # ... and the same through the path that rewrites the bf16 copies: p and ema carry every word; a copy is torch's rounding
    # of the value swapped in wherever that is a normal number, zero or inf, and NaN where it is NaN (a NaN's payload and the
    # rounding of a float denormal to bf16 are the converter's own)
    def p16_follows(i):
        now, lp = d["p"][i].cpu(), d["p16"][i].cpu()
        plain = ~torch.isnan(now) & ((now.abs() >= 2.0 ** -126) | (now == 0))
        assert torch.equal(_bits(lp[plain]), _bits(now.to(BF)[plain])), i
        assert torch.equal(torch.isnan(lp), torch.isnan(now)), i
    _swap(arena, d)
    for i in range(len(_sizes())):
        if d["p"][i].numel():
            assert torch.equal(_bits(d["p"][i]), snap[f"ema:{i}"]) and torch.equal(_bits(d["ema"][i]), snap[f"p:{i}"]), i
        if d["p16"][i] is not None and d["p16"][i].numel():
            p16_follows(i)
    _swap(arena, d)
    for k, t in _all(d).items():
        if not k.startswith("p16:"):
            assert torch.equal(_bits(t), snap[k]), k
    for i in WITH_P16:
        p16_follows(i)
    # update: an element is non-finite afterwards exactly where p or ema held NaN / inf; every other element obeys the bound
    _update(arena, d, 0.9)
    w = TBE.weight_at(0.9, 5)
    for i, (p, e) in enumerate(zip(h["p"], h["ema"])):
        if not p.numel():
            continue
        got = d["ema"][i].cpu()
        bad = ~(torch.isfinite(p) & torch.isfinite(e))
        assert torch.equal(~torch.isfinite(got), bad), i
        ref = e.double() + w * (p.double() - e.double())
        m = torch.maximum(torch.maximum(p.abs(), e.abs()).double(), ref.abs())
        ok = ~bad
        # (below the normal range a rounding is no longer relative: half a spacing of the denormals, 2^-150, for each of the
        # two roundings.  Denormals are not flushed: that would show here)
        assert bool(((got.double() - ref).abs()[ok] <= (BOUND(1, m) + 2.0 ** -149)[ok]).all()), i
        assert torch.equal(_bits(d["p"][i]), snap[f"p:{i}"]), i
    assert sum(len(v) for v in where["p"].values()) + sum(len(v) for v in where["ema"].values()) == 9


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(arena):
    from mimic_amd import ops
    h, _ = _host_set(5)
    d = _place(arena, h)
    snap = _snapshot(d)
    lib = ops.lib()
    p, e = d["p"][3], d["ema"][3]
    step = C.c_void_p(d["step"].data_ptr())

    def seg(pp, ee, n):
        return ops._EmaSeg(pp, ee, None, n)

    good = seg(p.data_ptr(), e.data_ptr(), p.numel())
    with outputs_in(arena):
        for bad in (1.0, -1e-3, float("nan"), float("inf")):
            with pytest.raises(ops.MopoeHipError, match="decay"):
                ops.ema_update(d["p"], d["ema"], bad, d["step"])
        cases = [("negative", [good, seg(p.data_ptr(), e.data_ptr(), -1)], 2),
                 ("NULL", [good, seg(None, e.data_ptr(), 5)], 2),
                 ("NULL", [good, seg(p.data_ptr(), None, 5)], 2),
                 ("bad arguments", [good], -1),
                 ("bad arguments", None, 1)]
        for why, recs, nseg in cases:
            arr = None if recs is None else (ops._EmaSeg * len(recs))(*recs)
            for rc in (lib.mopoe_ema_update(arr, nseg, C.c_double(0.9), step, None, ops._stream()),
                       lib.mopoe_ema_swap(arr, nseg, ops._stream())):
                assert rc == -1
                with pytest.raises(ops.MopoeHipError, match=why):
                    ops._check(rc)
        arr = (ops._EmaSeg * 1)(good)
        rc = lib.mopoe_ema_update(arr, 1, C.c_double(0.9), None, None, ops._stream())
        with pytest.raises(ops.MopoeHipError, match="step"):
            ops._check(rc)
    torch.cuda.synchronize()
    arena.assert_untouched()
    _same(d, snap)


# ---- 6. the whole model ------------------------------------------------------------------------------------------------------
MODEL_LR, DECAY = 1e-3, 0.9


def _build(decay=DECAY, max_norm=0.0, dp=False, compute_dtype="fp32", fixture="g0_s64"):
    """-> (exp, reducer, batches on the device, eps, cfg) for the fixture's tiny model in train_nodrop"""
    import mopoe_ref as R
    from golden_util import cfg_from, g0_state, load
    from model_util import build_exp
    g = load(fixture)
    if fixture.startswith("g7_"):
        from g7_util import g7_inputs
        cfg, sd, _, _, _ = g7_inputs(g)
    else:
        cfg, sd = cfg_from(g["cfg"]), g0_state(g)
    batches = [R.synthetic_batch(cfg, cfg.batch_size, seed=10 + i) for i in range(5)]
    eps = batches[0][1]
    exp = build_exp(cfg, sd, "cuda", "train_nodrop", eps=eps, compute_dtype=compute_dtype)
    exp.flags.initial_learning_rate = MODEL_LR
    exp.flags.ema_decay, exp.flags.max_grad_norm = decay, max_norm
    reducer = None
    if dp:
        from mimic_amd.parallel import GradAllReducer
        reducer = GradAllReducer(exp.mm_vae, 1, force=True)
        assert reducer.active
        reducer.broadcast_parameters()
    exp.set_optimizer()
    dev = [({k: v.cuda() for k, v in b[0].items()}, None) for b in batches]
    return exp, reducer, dev, eps, cfg


def _average_run(max_norm=0.0, dp=False):
    """two eager train steps, then the captured step (warmup=0) replayed three times; a snapshot of all parameters and of the
    step counter after every optimiser step -> worst |ema - fp64 recurrence| / bound over all elements, and what else the
    tests look at"""
    from mimic_amd import run_epochs as RE
    from mimic_amd.optim import HipAdam
    exp, reducer, dev, _, _ = _build(max_norm=max_norm, dp=dp)
    opt = exp.optimizer
    assert isinstance(opt, HipAdam) and opt.ema_decay == DECAY and (opt.clip_state is not None) == (max_norm > 0)
    early_calls = []
    real_early = opt.early_step
    opt.early_step = lambda *a, **k: (early_calls.append(1), real_early(*a, **k))[1]
    params = list(opt._params)
    ref = [p.detach().double().clone() for p in params]
    big = [p.detach().abs().double() for p in params]
    for e, p in zip(opt.ema_tensors(), params):
        assert torch.equal(e, p.detach())
    steps = []

    def snapshot():
        torch.cuda.synchronize()
        s = float(opt._step)
        steps.append(s)
        w = TBE.weight_at(DECAY, s)
        for i, p in enumerate(params):
            if p.grad is None:
                continue
            ref[i] = ref[i] + w * (p.detach().double() - ref[i])
            big[i] = torch.maximum(big[i], torch.maximum(p.detach().abs().double(), ref[i].abs()))

    pack = RE.ScalarPack(exp.flags.device)
    for i in (0, 1):
        RE.train_step(exp, dev[i], reducer, pack)
        snapshot()
    step = RE.GraphedTrainStep(exp, dev[0], pack, reducer, warmup=0)
    graph_opt = step.graph_opt is not None
    for i in (2, 3, 4):
        step(dev[i])
        snapshot()
    worst, no_grad_equal, n_no_grad = 0.0, True, 0
    for i, (p, e) in enumerate(zip(params, opt.ema_tensors())):
        if p.grad is None:
            n_no_grad += 1
            no_grad_equal = no_grad_equal and torch.equal(_bits(e), _bits(p.detach()))
            continue
        err = (e.double() - ref[i]).abs()
        worst = max(worst, float((err / BOUND(5, torch.maximum(big[i], e.abs().double())).clamp_min(1e-300)).max()))
    moved = max(float((e - p.detach()).abs().max()) for e, p in zip(opt.ema_tensors(), params))
    if reducer is not None:
        reducer.detach()
    return dict(worst=worst, steps=steps, no_grad_equal=no_grad_equal, n_no_grad=n_no_grad, early_calls=len(early_calls),
                graph_opt=graph_opt, moved=moved, skipped=None if opt.clip_state is None else float(opt.clip_state[3]))


def _check_run(r, what):
    print(f"model average [{what}]: worst |ema - ref| / bound = {r['worst']:.3f}; steps {r['steps']}; "
          f"{r['n_no_grad']} tensors without a gradient; early_step calls {r['early_calls']}")
    assert r["steps"] == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert r["worst"] <= 1.0, r["worst"]
    assert r["n_no_grad"] > 0 and r["no_grad_equal"]            # the word encoder's unused blocks: ema == p, bit for bit
    assert r["moved"] > 1e-4                                    # ... and everywhere else the average lags the weights


@pytest.mark.parametrize("form", ["early", "late", "clipped"])
def test_model_average_follows_eager_and_captured_steps(monkeypatch, form):
    from mimic_amd import run_epochs as RE
    assert RE.EARLY_ADAM, "MOPOE_EARLY_ADAM=0 in the environment: the default form is not what this test would run"
    if form == "late":
        monkeypatch.setattr(RE, "EARLY_ADAM", False)
    r = _average_run(max_norm=1.0 if form == "clipped" else 0.0)
    _check_run(r, form)
    assert (r["early_calls"] > 0) == (form == "early") and not r["graph_opt"]
    assert r["skipped"] == (0.0 if form == "clipped" else None)


# ---- 7. the data-parallel code path --------------------------------------------------------------------------------------------
def _dp_worker(rank, outdir):
    for p in PATHS:
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{os.path.join(outdir, 'rdzv')}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    torch.save(_average_run(dp=True), os.path.join(outdir, "out.pt"))
    dist.destroy_process_group()


def test_model_average_in_the_data_parallel_optimiser_graph():
    """one rank over RCCL with GradAllReducer(force=True): two eager steps, then the three-graph step whose optimiser graph
    holds the Adam and the EMA launches"""
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(d,), nprocs=1, join=True)
        r = torch.load(os.path.join(d, "out.pt"))
    _check_run(r, "data parallel")
    assert r["graph_opt"] and r["early_calls"] == 0


# ---- 8. evaluation and the checkpoint under the average --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluation_and_checkpoint_under_the_averaged_weights(tmp_path, dtype):
    from model_util import build_exp
    from mimic_amd import run_epochs as RE
    exp, _, dev, eps, cfg = _build(decay=0.5, compute_dtype=dtype, fixture="g0_s64" if dtype == "fp32" else "g7_small_bf16_nodrop")
    opt = exp.optimizer
    lowp = [] if opt.lowp is None else [(lp, p) for lp, p in zip(opt.lowp, opt._params) if lp is not None]
    assert bool(lowp) == (dtype == "bf16")
    for i in range(3):
        RE.train_step(exp, dev[i], None, None)
    loader = dev[3:5]
    live_scalars = RE.test(0, exp, loader)
    params = list(opt._params)
    state = lambda: ([_bits(p.detach()) for p in params] + [_bits(lp) for lp, _ in lowp]
                     + [_bits(opt._moments), _bits(opt._step), _bits(opt._ema_flat)])
    before = state()
    avg = [_bits(e) for e in opt.ema_tensors()]
    names = {k for k, _ in exp.mm_vae.named_buffers()}
    buffers = {k: v.detach().clone() for k, v in exp.mm_vae.state_dict().items() if k in names}
    with exp.averaged_weights() as on:
        assert on is True
        for p, a in zip(params, avg):
            assert torch.equal(_bits(p.detach()), a)
        for lp, p in lowp:
            assert torch.equal(_bits(lp), _bits(p.detach().reshape(-1).to(BF)))
        r1 = RE.test(0, exp, loader)
    for a, b in zip(state(), before):
        assert torch.equal(a, b)
    for lp, p in lowp:
        assert torch.equal(_bits(lp), _bits(p.detach().reshape(-1).to(BF)))
    assert math.isfinite(r1["total_loss"]) and r1["total_loss"] != live_scalars["total_loss"]
    again = RE.test(0, exp, loader)                                          # back on the live weights, the same scalars
    assert all(abs(v - again[k]) <= 2e-4 * abs(v) for k, v in live_scalars.items()), (live_scalars, again)
    # the checkpoint rule writes both files; the averaged one holds the reference's keys and loads strictly
    exp.flags.dir_checkpoints, exp.flags.end_epoch = str(tmp_path), 1
    RE.Callbacks(exp).save_checkpoint(0)
    for a, b in zip(state(), before):
        assert torch.equal(a, b)
    files = sorted(p.name for p in (tmp_path / "0000").iterdir())
    assert files == ["mm_vae", "mm_vae_ema"]
    live_sd = torch.load(tmp_path / "0000" / "mm_vae", map_location="cpu")
    ema_sd = torch.load(tmp_path / "0000" / "mm_vae_ema", map_location="cpu")
    assert list(live_sd) == list(ema_sd)
    named_buffers = set(buffers)
    assert named_buffers and named_buffers < set(ema_sd)
    for k in named_buffers:                                                  # BatchNorm buffers: the live model's
        assert torch.equal(ema_sd[k], buffers[k].cpu()) and torch.equal(ema_sd[k], live_sd[k]), k
    assert any(not torch.equal(ema_sd[k], live_sd[k]) for k in ema_sd if k not in named_buffers)
    exp2 = build_exp(cfg, ema_sd, "cuda", "eval", eps=eps, compute_dtype=dtype)      # (load_state_dict(strict=True) inside)
    r2 = RE.test(0, exp2, loader)
    for k, v in r1.items():
        print(f"{dtype} {k}: averaged in place {v!r}, from mm_vae_ema {r2[k]!r}")
        assert abs(v - r2[k]) <= 2e-4 * abs(v), (k, v, r2[k])


# ---- 9. the launcher -------------------------------------------------------------------------------------------------------------
def test_two_averaged_epochs_on_tensor_files_through_the_launcher(tmp_path):
    """tests/test_launcher_gpu.py: test_two_epochs_on_tensor_files_through_the_launcher with --ema_decay 0.9 and the
    latent-representation evaluation at every epoch"""
    from golden_util import make_mimic_files
    from mimic_amd import main_mimic as MM
    from mimic_amd.utils.experiment import HotPathExperiment
    data = tmp_path / "data"
    make_mimic_files(str(data), img_size=64, n_train=100, n_eval=30, seed=5)
    run_dir = tmp_path / "run"
    flags = MM.parse_flags(["--dataset", "mimic", "--dir_data", str(data), "--img_size", "64", "--class_dim", "32",
                            "--DIM_img", "64", "--DIM_text", "32", "--batch_size", "8", "--len_sequence", "128",
                            "--end_epoch", "2", "--initial_learning_rate", "1e-5", "--ema_decay", "0.9", "--eval_freq", "1",
                            "--eval_lr", "true", "--num_training_samples_lr", "50", "--dir_experiment_run", str(run_dir)])
    assert flags.ema_decay == 0.9
    m = MM.Main(flags)
    m.setup_distributed = lambda: (setattr(m.flags, "world_size", 1), setattr(m.flags, "distributed", False))
    assert m.main() is True and m.current_tries == 0
    hist = m.history
    assert [h["epoch"] for h in hist] == [0, 1]
    n_train = hist[0]["train"]["steps"]
    assert hist[1]["train"]["graphed_steps"] >= n_train - 1               # the step with the average is still the captured one
    for h in hist:
        assert h["test"]["weights"] == "ema" and math.isfinite(h["test"]["total_loss"]) and "lr_eval" in h["test"]
    line = MM.result_line(hist)
    assert line["eval_weights"] == "ema" and "last_lr_eval" in line
    ckpt = run_dir / "checkpoints" / "0001"
    live_sd = torch.load(ckpt / "mm_vae", map_location="cpu")
    ema_sd = torch.load(ckpt / "mm_vae_ema", map_location="cpu")
    f = copy.copy(m.flags)
    f.device = torch.device("cpu")
    fresh = HotPathExperiment(f).mm_vae
    fresh.load_state_dict(live_sd, strict=True)
    fresh.load_state_dict(ema_sd, strict=True)
    assert list(live_sd) == list(ema_sd)
    assert any(not torch.equal(live_sd[k], ema_sd[k]) for k in live_sd)
