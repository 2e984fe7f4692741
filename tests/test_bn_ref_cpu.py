"""Host-side validation of a mopoe_bn_ref (csrc/bn_ref_check.hpp: check_bn_ref, the code every entry point that takes a
reference runs before it enqueues anything) against an independent restatement in Python, on the CPU:
tests/tools/bn_ref_shim.cpp is built with the host compiler, loaded with ctypes, and nothing is launched.

  * the full product of modes -1..4, each of the five pointers present or absent, inv_count in {0, 1/7, inf, nan, -1}, C equal
    or unequal to the entry point's channel count, mode 3 allowed or not (+ the NULL reference);
  * every refusal is MOPOE_ERR_ARG with a message that names the entry point;
  * the mode-3 accuracy test's CPU half (tests/bn_mode3_cases.py): the fp32 emulation of conv_dgrad with a mode-3 reference
    meets, against fp64, the assertions the bf16 kernel is held to in tests/test_bn_modes_gpu.py, on the same inputs -- so
    the inputs leave the reference itself inside the derived bound.
"""
import ctypes
import itertools
import math
import os
import shutil
import subprocess

import pytest
import torch

import bn_mode3_cases as M3
import torch_backend as TB

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "tools", "bn_ref_shim.cpp")
ERR_ARG = -1
WHO = "mopoe_some_entry_point: bn_arg"
POINTERS = ("sums", "gamma", "beta", "rmean", "rvar")      # bit i of `present`


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("bn_ref") / "bn_ref_shim.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, SHIM_SRC])
    lib = ctypes.CDLL(so)
    lib.shim_check_bn_ref.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    return lib


def expected_ok(null_ref, mode, present, inv_count, c, expected_c, allow3):
    """the rules of the issue, restated: is this reference accepted?"""
    if null_ref or mode == 0:
        return True                                      # absent
    has = dict(zip(POINTERS, present))
    if mode not in (1, 2, 3):
        return False
    if mode == 3 and not allow3:
        return False
    if not (has["gamma"] and has["beta"]) or c != expected_c:
        return False
    if mode == 1:
        return has["sums"] and math.isfinite(inv_count) and inv_count > 0
    if mode == 2:
        return has["rmean"] and has["rvar"]
    return True                                          # mode 3: nothing more


def call(lib, null_ref, mode, present, inv_count, c, expected_c, allow3):
    msg = ctypes.create_string_buffer(256)
    bits = sum(1 << i for i, p in enumerate(present) if p)
    rc = lib.shim_check_bn_ref(int(null_ref), mode, bits, inv_count, c, expected_c, int(allow3), WHO.encode(), msg, len(msg))
    return rc, msg.value.decode()


def test_check_bn_ref_against_the_rules(shim):
    n_ok = n_refused = 0
    for mode, present, inv_count, c, allow3 in itertools.product(
            range(-1, 5), itertools.product((False, True), repeat=5), (0.0, 1.0 / 7, math.inf, math.nan, -1.0), (64, 32), (False, True)):
        rc, msg = call(shim, False, mode, present, inv_count, c, 64, allow3)
        want = expected_ok(False, mode, present, inv_count, c, 64, allow3)
        assert rc == (0 if want else ERR_ARG), (mode, present, inv_count, c, allow3, rc, msg)
        if want:
            n_ok += 1
        else:
            n_refused += 1
            assert WHO in msg, (mode, present, inv_count, c, allow3, msg)
    assert n_ok > 0 and n_refused > 0
    # a NULL reference is "absent", whatever else is asked
    for allow3 in (False, True):
        assert call(shim, True, 7, (False,) * 5, math.nan, 1, 64, allow3)[0] == 0


def test_refusal_messages_name_the_field(shim):
    full = (True,) * 5
    for mode, missing in ((1, "sums"), (1, "gamma"), (2, "beta"), (2, "rmean"), (2, "rvar"), (3, "gamma"), (3, "beta")):
        present = tuple(p != missing for p in POINTERS)
        rc, msg = call(shim, False, mode, present, 0.5, 64, 64, True)
        assert rc == ERR_ARG and WHO in msg and missing in msg, (mode, missing, msg)
    assert "inv_count" in call(shim, False, 1, full, 0.0, 64, 64, False)[1]
    assert "mode 7" in call(shim, False, 7, full, 0.5, 64, 64, True)[1]
    assert "mode 3" in call(shim, False, 3, full, 0.5, 64, 64, False)[1]
    rc, msg = call(shim, False, 2, full, 0.5, 32, 64, False)
    assert rc == ERR_ARG and "C = 32" in msg and "64" in msg, msg
    # mode 3 reads gamma and beta alone: no statistics of either kind, no count
    assert call(shim, False, 3, (False, True, True, False, False), 0.0, 64, 64, True) == (0, "")


@pytest.mark.parametrize("gabs,beta", M3.SETTINGS, ids=[f"gamma{g}_beta{b}" for g, b in M3.SETTINGS])
def test_mode3_emulation_meets_the_bound_against_fp64(gabs, beta):
    case = M3.Mode3Case(gabs, beta)
    # the two fp64 references themselves differ by no more than the derived slack
    d = (case.ref_stored["sums"][1] - case.ref_exact["sums"][1]).abs()
    assert (d <= case.slack).all(), (d / case.slack).max().item()
    sums = torch.zeros(2, M3.GEOM.Cin, dtype=torch.float64)
    dx = TB.conv_dgrad(case.dy, case.w, M3.GEOM, relu_bn=case.bn2y, xin=case.a2, bwd_sums=sums)
    assert dx.dtype == M3.BF
    M3.assert_mode3(case, dx, sums, f"emulation |gamma|={gabs} beta={beta}")
