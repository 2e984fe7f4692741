"""The guard-band arena (tests/arena.py) itself, the coverage table of tests/test_guarded_ops_gpu.py against the header, and the
hostile-value input sets of tests/hostile_sets.py on the CPU: on every set the fp32 reference arithmetic (tests/torch_backend*.py,
or torch's own batch_norm) stays within HALF of the bar the GPU test uses when compared with its own fp64 evaluation -- so a
GPU failure on these sets is the kernel's, not the yardstick's.  Sets as pinned here (none had to be narrowed):

  * BatchNorm at shifted means: rows x 64 with rows in (65536, 4096), randn + r for r in (0, 10, 30, 100), and the same with
    channel 5 scaled by 1e-2; gated for r <= 30;
  * degenerate channels: a constant column, gamma == 0 (modes 1 and 3), running variance 0 (mode 2), on ragged_c20 and a
    64-channel vector geometry;
  * latent kernels: mu ~ 3 randn, logvar uniform in [-8, 8].
"""
import ast
import os
import re

import pytest
import torch

import hostile_sets as HS
import torch_backend as TB
import torch_backend_lhood as TBL
import torch_backend_lr as TBLR
import torch_backend_methods as TBM
import torch_backend_style as TBS
from arena import Arena, ArenaError, MIN_GUARD, outputs_in
from mimic_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.fixture
def arena():
    return Arena("cpu", capacity=24 << 20, capacity64=8 << 20)


def test_placement_alignment_and_guards(arena):
    gen = torch.Generator().manual_seed(0)
    a = torch.randn(37, 20, generator=gen)
    b = torch.randn(5, 640, generator=gen).to(BF)
    c = torch.randn(2, 20, generator=gen, dtype=torch.float64)
    va, vb, vc = arena.place(a), arena.place(b, misalign_bytes=8), arena.place(c, misalign_bytes=8)
    vd = arena.place(a, misalign_bytes=4)
    for v, t, off in ((va, a, 0), (vb, b, 8), (vc, c, 8), (vd, a, 4)):
        assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous() and torch.equal(v, t)
        assert v.data_ptr() % 16 == off
    base = arena.raw["h"].data_ptr()
    assert va.data_ptr() - base >= MIN_GUARD                                      # a guard in front of the first view
    assert vb.data_ptr() - (va.data_ptr() + a.numel() * 4) >= MIN_GUARD           # ... and between two views
    assert base + arena.raw["h"].numel() - (vd.data_ptr() + a.numel() * 4) >= MIN_GUARD
    wide = torch.zeros(3, 2008)                                                   # 256 rows of 2008 floats exceed 1 MiB
    assert Arena.guard_bytes(wide.shape, wide.dtype) == 256 * 2008 * 4
    vw = arena.place(wide)
    assert vw.data_ptr() - (vd.data_ptr() + a.numel() * 4) >= 256 * 2008 * 4
    arena.assert_untouched()
    with pytest.raises(AssertionError):
        arena.place(b, misalign_bytes=3)                                          # not a multiple of the element size
    with pytest.raises(ArenaError, match="arena full"):
        arena.place(torch.zeros(8 << 20))
    arena.reset()
    assert not arena.views
    arena.assert_untouched()


def test_the_poison_reads_as_nan_in_every_type(arena):
    for dtype in (torch.float32, BF, torch.float64):
        out = arena.new_output((7, 9), dtype)
        assert bool(torch.isnan(out).all()), dtype
        assert arena.is_poison(out)
    z = arena.new_output((4, 3), torch.float32, zero=True)
    assert not bool(z.any()) and not arena.is_poison(z)
    raw = arena.raw["h"]
    assert bool(torch.isnan(raw[:4096].view(torch.float32)).all()) and bool(torch.isnan(raw[:4096].view(BF)).all())
    assert bool(torch.isnan(arena.raw["d"][:4096].view(torch.float64)).all())


@pytest.mark.parametrize("where", ["before", "after", "between", "fp64"])
def test_a_single_changed_byte_is_reported(arena, where):
    a = arena.place(torch.ones(10, 6), name="first")
    b = arena.place(torch.ones(3, 8), name="second")
    d = arena.place(torch.ones(5, dtype=torch.float64), name="stats")
    arena.assert_untouched()
    raw, raw64 = arena.raw["h"], arena.raw["d"]
    off_a, off_b = a.data_ptr() - raw.data_ptr(), b.data_ptr() - raw.data_ptr()
    if where == "before":
        raw[off_a - 3] = 0
        msg = "3 bytes before the start of view 'first'"
    elif where == "after":
        raw[off_b + 3 * 8 * 4 + 100] = 0x55
        msg = "100 bytes past the end of view 'second'"
    elif where == "between":
        raw[off_a + 240 + 17] ^= 0xFF                       # one byte of the guard between the two views, nearer the first
        msg = "17 bytes past the end of view 'first'"
    else:
        raw64[d.data_ptr() - raw64.data_ptr() - 8] = 1
        msg = "8 bytes before the start of view 'stats'"
    with pytest.raises(ArenaError, match=msg):
        arena.assert_untouched()
    a.fill_(3.0)                                            # writes INSIDE a view are the tensor's own business
    arena.reset()
    arena.assert_untouched()


def test_outputs_in_routes_ops_allocations_and_restores_torch(arena):
    real = ops.torch
    dev = torch.device("cpu")
    with outputs_in(arena) as px:
        assert ops.torch is px and ops.torch.float32 is torch.float32 and ops.torch.Tensor is torch.Tensor
        e = ops.torch.empty((3, 5), dtype=torch.float32, device=dev)
        e2 = ops.torch.empty(2, 3, 4, dtype=BF, device=dev)
        z = ops.torch.zeros(4, 7, dtype=torch.float32, device=dev)
        z64 = ops.new_stats(6, dev)                         # the zeros that receive statistics: still zero-filled
        like = ops.torch.empty_like(e2)
        assert all(arena.owns(t) for t in (e, e2, z, z64, like)) and len(px.allocated) == 5
        assert bool(torch.isnan(e).all()) and bool(torch.isnan(e2).all()) and bool(torch.isnan(like).all())
        assert not bool(z.any()) and z64.dtype == torch.float64 and tuple(z64.shape) == (2, 6) and not bool(z64.any())
        assert like.shape == e2.shape and like.dtype == BF
        elsewhere = ops.torch.empty(3, dtype=torch.float32, device="meta")       # another device: forwarded
        assert not arena.owns(elsewhere)
        with pytest.raises(ArenaError, match="memory_format"):                   # a request the proxy cannot restate is refused
            ops.torch.empty_like(e2, memory_format=torch.contiguous_format)
        with pytest.raises(ArenaError, match="requires_grad"):
            ops.torch.zeros(3, dtype=torch.float32, device=dev, requires_grad=False)
        assert len(px.allocated) == 5
    assert ops.torch is real
    with pytest.raises(RuntimeError, match="boom"):
        with outputs_in(arena):
            raise RuntimeError("boom")
    assert ops.torch is real
    arena.assert_untouched()


# ---- the coverage table of the GPU file against the header -------------------------------------------------------------------
EXEMPT = {"mopoe_abi_version", "mopoe_last_error", "mopoe_conv_workspace_bytes", "mopoe_prof_enable", "mopoe_prof_stamp", "mopoe_prof_collect"}


def test_every_entry_point_that_writes_device_memory_is_in_the_guarded_table():
    header = open(os.path.join(REPO, "include", "mopoe_hip.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b(mopoe_[a-z0-9_]+)\s*\(", decls))
    assert len(names) > 60 and EXEMPT <= names, sorted(EXEMPT - names)
    src = open(os.path.join(REPO, "tests", "test_guarded_ops_gpu.py")).read()
    doc = src.split('"""')[1]
    table = dict(re.findall(r"^\s+(mopoe_[a-z0-9_]+)\s+->\s+(test_[a-z0-9_]+)\s*$", doc, flags=re.M))
    assert not (names - EXEMPT - set(table)), f"entry points without a guarded case: {sorted(names - EXEMPT - set(table))}"
    assert not (set(table) - names), f"the table names entry points the header does not have: {sorted(set(table) - names)}"
    for fn in EXEMPT:
        assert fn in doc, f"{fn}: exempt without a stated reason"
    tests = set(re.findall(r"^def (test_[a-z0-9_]+)\(", src, flags=re.M))
    assert set(table.values()) <= tests, sorted(set(table.values()) - tests)
    # ... and the wrapper each row stands for is called in the body of THAT test, or of a helper of the file reachable from it
    # (what was really launched is judged on the GPU: test_every_row_of_the_table_was_called_by_its_test)
    funcs = {n.name: n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}

    def wrappers(name, seen):
        seen.add(name)
        found = set()
        for node in ast.walk(funcs[name]):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) \
                    and node.func.value.id in ("ops", "f"):
                found.add(node.func.attr)
            elif isinstance(node, ast.Name) and node.id in funcs and node.id not in seen:
                found |= wrappers(node.id, seen)
        return found
    reach = {test: wrappers(test, set()) for test in set(table.values())}
    for fn, test in table.items():
        op = fn[len("mopoe_"):]
        for suffix in ("_bf16out", "_bf16"):
            op = op[:-len(suffix)] if op.endswith(suffix) else op
        op = {"conv_fwd_mix": "conv_fwd", "edge_expand": "conv_fwd", "edge_reduce": "conv_fwd", "edge_wgrad": "conv_wgrad"}.get(op, op)
        assert op in reach[test], (fn, op, test)
    assert "latent_fwd" not in reach["test_adam_step"]          # (the walk does not simply reach everything)


# ---- the hostile-value sets: the references within half of the GPU bars ----------------------------------------------------------
@pytest.mark.parametrize("rows", HS.BN_SHIFT_ROWS)
@pytest.mark.parametrize("narrow", [False, True])
def test_batch_norm_reference_error_at_shifted_means(rows, narrow):
    """the GPU gate is 4 x (error of torch's fp32 batch_norm + autograd against fp64) + the floor of check: for the gated
    shifts that reference error stays below half of the floor, i.e. the gate is never looser than 3 floors"""
    for r in HS.BN_SHIFTS:
        ref = HS.bn_reference_errors(HS.bn_shift_inputs(rows, 64, r, narrow))
        for k, floor in HS.BN_FLOOR.items():
            e = ref["ref_err"][k]
            assert e == e and e < float("inf"), (r, k)
            if r <= HS.BN_GATED_SHIFT:
                assert e <= 0.5 * floor, (rows, r, narrow, k, e, floor)


@pytest.fixture
def references_at_half_bar(monkeypatch):
    """tests/test_guarded_ops_gpu.py with mimic_amd.ops routed to the fp32 references on the CPU and every bar halved: what its
    harness then compares is the fp32 reference with the reference's fp64 evaluation"""
    import test_guarded_ops_gpu as G
    import test_hip_ops_gpu as H
    monkeypatch.setattr(G, "DEV", "cpu")
    monkeypatch.setattr(G, "BAR_SCALE", 0.5)
    monkeypatch.setattr(G, "_log", lambda msg: None)
    monkeypatch.setattr(H, "_log", lambda msg: None)
    for mod in (TB, TBM, TBS, TBL, TBLR):
        mod.install(monkeypatch)
    ws = torch.zeros(1 << 20, dtype=torch.uint8)
    monkeypatch.setattr(ops, "_workspace", lambda device: (ws, ws.numel()))
    monkeypatch.setattr(ops, "_kl_ws", {})
    return G, Arena("cpu", capacity=160 << 20, capacity64=24 << 20)


@pytest.mark.parametrize("name", ["ragged_c20", "vector_c64"])
@pytest.mark.parametrize("case", HS.DEGENERATE_CASES)
def test_references_on_degenerate_channels(references_at_half_bar, name, case):
    G, arena = references_at_half_bar
    G.test_degenerate_channels(arena, name, case)


def test_references_at_wide_logvariances(references_at_half_bar):
    G, arena = references_at_half_bar
    G.test_latent_kernels_at_wide_logvariances(arena)
