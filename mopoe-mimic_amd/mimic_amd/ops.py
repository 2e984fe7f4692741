"""ctypes binding of libmopoe_hip.so (include/mopoe_hip.h): the ONLY compute backend of mimic_amd.

There is deliberately no CPU / eager fallback here: if the HIP library is missing or the tensors are
not on a GPU the ops raise.  (CPU tests of the host logic monkeypatch this module's functions with
the torch emulation under tests/, which is test infrastructure, not a product path.)

Every function takes/returns channels-last tensors (see the header for the layout contract): fp32, or -- the bf16
storage family of BASELINE configs #3 / #5 -- bfloat16 activations and bf16 weight copies with fp32 accumulation; the
entry point is chosen by the dtype of the activation operand.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOPOE_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libmopoe_hip.so")  # env override: A/B builds
ABI_VERSION = 25

RES_A, RES_B = 2.0, 0.3
BN_EPS = 1e-5
SUBSET_MASKS = (1, 2, 4, 3, 5, 6, 7)  # bit0 PA, bit1 Lateral, bit2 text; reference subset order


class MopoeHipError(RuntimeError):
    pass


# ----------------------------------------------------------------------------------------------
# plain-data descriptors shared with the C ABI
# ----------------------------------------------------------------------------------------------
class _Geom(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("N", "Hs", "Ws", "Hb", "Wb", "Cin", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "transposed")]


class _BnRef(C.Structure):
    _fields_ = [("sums", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("rmean", C.c_void_p),
                ("rvar", C.c_void_p), ("inv_count", C.c_double), ("eps", C.c_float), ("C", C.c_int32),
                ("mode", C.c_int32)]


class _MaskRef(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("kind", C.c_int32), ("rows_per_sample", C.c_int32)]


class _MixRef(C.Structure):   # mopoe_mix_ref
    _fields_ = [("s", C.c_void_p), ("bn", _BnRef), ("a", C.c_float), ("b", C.c_float)]


class _RunDesc(C.Structure):
    _fields_ = [("sums", C.c_void_p), ("rmean", C.c_void_p), ("rvar", C.c_void_p), ("C", C.c_int32),
                ("count", C.c_int32)]


class _AdamSeg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("p16", C.c_void_p),
                ("n", C.c_int64)]


class _EmaSeg(C.Structure):   # mopoe_ema_seg (include/mopoe_hip_ema.h)
    _fields_ = [("p", C.c_void_p), ("ema", C.c_void_p), ("p16", C.c_void_p), ("n", C.c_int64)]


@dataclass(frozen=True)
class Geom:
    """Conv / ConvTranspose geometry; 'small' grid = conv output / convT input (header: mopoe_conv_geom)."""
    N: int
    Hs: int
    Ws: int
    Hb: int
    Wb: int
    Cin: int
    Cout: int
    kh: int
    kw: int
    sh: int
    sw: int
    ph: int
    pw: int
    transposed: bool

    def __post_init__(self):
        object.__setattr__(self, "_hash", hash((self.N, self.Hs, self.Ws, self.Hb, self.Wb, self.Cin, self.Cout, self.kh,
                                                self.kw, self.sh, self.sw, self.ph, self.pw, self.transposed)))

    def __hash__(self):   # Geoms key the plan / struct caches on every launch: hash once
        return self._hash

    @property
    def in_shape(self):
        return (self.N, self.Hs, self.Ws, self.Cin) if self.transposed else (self.N, self.Hb, self.Wb, self.Cin)

    @property
    def out_shape(self):
        return (self.N, self.Hb, self.Wb, self.Cout) if self.transposed else (self.N, self.Hs, self.Ws, self.Cout)

    @property
    def taps(self):
        return self.kh * self.kw

    def with_batch(self, n):
        return _with_batch(self, n)

    def c(self):
        return _geom_struct(self)


@lru_cache(maxsize=None)
def _with_batch(g: "Geom", n: int) -> "Geom":
    return Geom(n, *[getattr(g, f) for f in
                     ("Hs", "Ws", "Hb", "Wb", "Cin", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "transposed")])


@lru_cache(maxsize=None)
def _geom_struct(g: "Geom") -> "_Geom":
    return _Geom(g.N, g.Hs, g.Ws, g.Hb, g.Wb, g.Cin, g.Cout, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, int(g.transposed))


@dataclass
class Bn:
    """A BatchNorm to be applied / inverted inside another kernel (header: mopoe_bn_ref)."""
    gamma: torch.Tensor
    beta: torch.Tensor
    mode: int                               # 1 batch statistics, 2 running statistics, 3 = the ACTIVATION is xin (conv_dgrad): gamma, beta only
    sums: Optional[torch.Tensor] = None     # double [2, C] (mode 1)
    count: int = 0                          # rows the sums were taken over (mode 1)
    rmean: Optional[torch.Tensor] = None
    rvar: Optional[torch.Tensor] = None
    eps: float = BN_EPS

    def c(self):
        return _BnRef(_p(self.sums), _p(self.gamma), _p(self.beta), _p(self.rmean), _p(self.rvar),
                      (1.0 / self.count) if self.count else 0.0, self.eps, self.gamma.numel(), self.mode)


@dataclass
class Mask:
    """Dropout multiplier (values 0 or 2).  kind 1: [N, C] per-sample channel mask (nn.Dropout2d);
    kind 2: [rows, C] elementwise (nn.Dropout)."""
    mask: torch.Tensor
    kind: int
    rows_per_sample: int = 1

    def c(self):
        return _MaskRef(_p(self.mask), self.kind, self.rows_per_sample)


_NO_BN = _BnRef(None, None, None, None, None, 0.0, 0.0, 0, 0)
_NO_MASK = _MaskRef(None, 0, 1)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------
# library loading
# ----------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MopoeHipError(f"{LIB_PATH} not built: run `python __graft_entry__.py build` "
                                "(mimic_amd has no CPU fallback)")
        _lib = C.CDLL(LIB_PATH)
        _lib.mopoe_last_error.restype = C.c_char_p
        _lib.mopoe_abi_version.restype = C.c_int
        if _lib.mopoe_abi_version() != ABI_VERSION:
            raise MopoeHipError("libmopoe_hip.so ABI version mismatch")
    return _lib


def _check(rc: int):
    if rc != 0:
        raise MopoeHipError(f"libmopoe_hip error {rc}: {lib().mopoe_last_error().decode()}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(device=None) -> int:
    """current HIP stream of the device as an integer (fast path: torch.cuda.current_stream() costs ~7 us)"""
    if _raw_stream is not None:
        idx = torch.cuda.current_device() if device is None or device.index is None else device.index
        return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream


def _stream():
    return C.c_void_p(_stream_ptr())


def _dev(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise MopoeHipError("mimic_amd ops need GPU tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise MopoeHipError("mimic_amd ops need contiguous tensors")


def _bn(bn: Optional[Bn]):
    return C.byref(bn.c()) if bn is not None else C.byref(_NO_BN)


def _mask(m: Optional[Mask]):
    return C.byref(m.c()) if m is not None else C.byref(_NO_MASK)


_conv_ws = {}


def _workspace(device):
    """Per-device scratch for the split reductions of small-grid conv layers (C ABI: caller-owned)."""
    key = (device.index, _stream_ptr(device))
    if key not in _conv_ws:
        lib().mopoe_conv_workspace_bytes.restype = C.c_size_t
        nbytes = int(lib().mopoe_conv_workspace_bytes())
        _conv_ws[key] = (torch.zeros(nbytes, dtype=torch.uint8, device=device), nbytes)   # (arrival counters start at zero)
    return _conv_ws[key]


def new_stats(n_channels: int, device) -> torch.Tensor:
    return torch.zeros(2, n_channels, dtype=torch.float64, device=device)


# ----------------------------------------------------------------------------------------------
# convolution family
# ----------------------------------------------------------------------------------------------
class _Plan(C.Structure):
    """header: mopoe_conv_plan"""
    _fields_ = [("tile", C.c_int32), ("split", C.c_int32)]


# Launch plans.  The library has a static tile / split heuristic; the mirror can do better by measuring: the
# first time a (op, geometry, fusion) triple is met (i.e. during the first warm-up step) every candidate plan
# is launched a few times on scratch accumulators, timed with events on the current stream, and the fastest is
# kept for the life of the process.  All plans compute the same sums (in a different association order).
# MOPOE_AUTOTUNE=0 keeps the static heuristic (plan = NULL).
AUTOTUNE = os.environ.get("MOPOE_AUTOTUNE", "1") not in ("0", "table")
# MOPOE_AUTOTUNE=table: the committed plans where the table has the triple, the static heuristic elsewhere, no timing at all
# (the GPU tests of the BASELINE shapes run in this mode: the kernels the product launches, without a tuner pass per test)
TABLE_ONLY = os.environ.get("MOPOE_AUTOTUNE", "1") == "table"
_TUNE_REPS = int(os.environ.get("MOPOE_TUNE_REPS", "3"))
# Optional: leave the first N conv launches of the process on the static heuristic and start tuning afterwards
# (a GPU that has just left idle ranks candidates differently from steady state).  Default 0 = tune at first use,
# so that one warm-up step settles every plan.
TUNE_AFTER_CALLS = int(os.environ.get("MOPOE_TUNE_AFTER_CALLS", "0"))
# Objective of the ranking: duration x (alpha + (1 - alpha) x the fraction of the chip the launch occupies).  1.0 = isolated
# latency alone.  0.7 (default since round 4): inside the step three networks' kernels share the chip, and a plan that is a few
# per cent slower alone but leaves CUs (and LDS) to the other branches wins there -- force-tuned bench.py, same box:
# C2 6 305 / 6 312 (1.0) -> 6 444 / 6 451 / 6 473 (0.7), 6 440 (0.6), 6 342 (0.5), 6 018 (0.3); C5 5 100 -> 5 239; c2d128 2 671 -> 2 707;
# C3 22 677 -> 22 761
TUNE_ALPHA = float(os.environ.get("MOPOE_TUNE_ALPHA", "0.7"))
# tiles 8..11 (LDS-free kernel) among the tuner's candidates: off by default -- they win on many small layers when timed
# alone but the step as a whole (three modalities' kernels running side by side) is not faster with them
DIRECT_TILES = os.environ.get("MOPOE_DIRECT_TILES", "0") != "0"
_conv_calls = 0
_plans = {}
F32_GLDS = os.environ.get("MOPOE_F32_GLDS", "1") != "0"       # A/B switch: keep the tuner off the LDS-DMA tiles
# A/B switch: tiles 16..19 (plain operand) offered.  The products are the same fp32 numbers -- each operand is split exactly
# into three bf16 parts and six of the nine partial products are accumulated in fp32 by v_mfma_f32_32x32x16_bf16; the error
# against fp64 is lower than that of v_mfma_f32_32x32x2_f32 (csrc/conv_gemm_glds.inc, tests: test_f32_products_on_the_bf16_pipe)
F32_SPLIT_BF16 = os.environ.get("MOPOE_F32_SPLIT_BF16", "1") != "0"
BF16_GLDS = os.environ.get("MOPOE_BF16_GLDS", "1") != "0"      # A/B switch: keep the tuner on the register-staged tiles
WGRAD_PARITY = os.environ.get("MOPOE_WGRAD_PARITY", "1") != "0"  # A/B switch: wgrad tile 8 (four taps per block) offered
_SPLITS = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)

# ---- the conv tiles: one table per family with every fact the tuner, the F32_SPLIT_BF16 remap and the profiling names need,
# once per tile.  The rows restate csrc/conv_launch.hpp (MOPOE_*_TILES); tests/test_conv_launch_cpu.py holds them against that
# header, tests/test_abi_cpu.py the names built from them against the kernels of the built library.
#   kernel      GatherKernel of the header without its G_ (HNONE: a number kept for a tile that is not built)
#   targs       template arguments of the instantiations, {} = spec: 1 forward, plain operand | 2 forward, BN -> ReLU on load |
#               3 input gradient | 0 run-time flags (K no multiple of the chunk); scalar_targs: the scalar-path form
#   k_multiple  the tile is offered only where the K channels are a multiple of this (its K chunk; 1: any K)
#   vec_only    no scalar-path form: channel counts % 4 == 0;  switches: the A/B switches above that must all be on
#   bn_form     a BN -> ReLU-on-load instantiation exists (else: plain operands only)
#   kind        first profiling kind; kind_bn: the BN-on-load form of a bf16 LDS-DMA tile
#   tuner_resident  blocks the TUNER takes to fill the chip: the denominator of the occupancy term of its objective.  NOT the
#               header's `persist`, the launcher's cap on a persistent grid (2048 / 3072 on the fp32 register-staged tiles where
#               this says 512 / 768).  The committed plans were ranked with these numbers: do not "correct" them
#   twin        with F32_SPLIT_BF16 off, the tile a committed plan on this one is launched as
_GatherTile = namedtuple("_GatherTile", "kernel id bm bn targs k_multiple vec_only switches bn_form kind tuner_resident "
                                        "scalar_targs kind_bn twin", defaults=(None, None, None))
_F32_GATHER_TILES = (
    _GatherTile("LDS_S", 0, 128, 128, "128, 128, 2, 4, 16, true, {}", 1, False, "", True, 0, 512, "128, 128, 2, 2, 16, false, 0"),
    _GatherTile("LDS_S", 1, 256, 64, "256, 64, 4, 2, 16, true, {}", 1, False, "", True, 4, 512, "256, 64, 4, 1, 16, false, 0"),
    _GatherTile("LDS_S", 2, 64, 64, "64, 64, 2, 2, 16, true, {}", 1, False, "", True, 8, 768, "64, 64, 2, 2, 16, false, 0"),
    _GatherTile("LDS", 3, 256, 128, "256, 128, 4, 2, 16, true, {}", 1, True, "", True, 12, 512),
    _GatherTile("LDS", 4, 128, 64, "128, 64, 2, 2, 16, true, {}", 1, True, "", True, 16, 768),
    _GatherTile("LDS", 5, 64, 64, "64, 64, 2, 2, 32, true, {}", 32, True, "", True, 20, 768),
    _GatherTile("LDS", 6, 128, 64, "128, 64, 2, 2, 32, true, {}", 32, True, "", True, 24, 768),
    _GatherTile("LDS", 7, 128, 128, "128, 128, 2, 2, 16, true, {}", 1, True, "", True, 28, 768),
    # 8..11: the LDS-free kernel (off by default, see DIRECT_TILES)
    _GatherTile("DIRECT", 8, 128, 128, "2, 2, 2, 2, {}", 8, True, "DIRECT_TILES", True, 44, 768),
    _GatherTile("DIRECT", 9, 256, 64, "4, 1, 2, 2, {}", 8, True, "DIRECT_TILES", True, 48, 768),
    _GatherTile("DIRECT", 10, 64, 64, "2, 2, 1, 1, {}", 8, True, "DIRECT_TILES", True, 52, 768),
    _GatherTile("DIRECT", 11, 128, 64, "2, 1, 2, 2, {}", 8, True, "DIRECT_TILES", True, 56, 768),
    # 12..15: the LDS-DMA family (csrc/conv_gemm_glds.inc); with BN on load: the tiles with 2 or 4 buffers
    _GatherTile("GLDS", 12, 128, 128, "128, 128, 2, 2, {}, 2, 1, 0", 32, True, "F32_GLDS", True, 104, 512),
    _GatherTile("GLDS", 13, 128, 64, "128, 64, 2, 2, {}, 3, 1, 0", 32, True, "F32_GLDS", False, 107, 512),
    _GatherTile("GLDS", 14, 64, 64, "64, 64, 2, 2, {}, 4, 1, 0", 32, True, "F32_GLDS", True, 110, 512),
    _GatherTile("GLDS", 15, 256, 128, "256, 128, 4, 2, {}, 2, 1, 0", 32, True, "F32_GLDS", True, 113, 256),
    # 16..19: the same with the fp32 products on the bf16 matrix pipe
    _GatherTile("EMU", 16, 128, 128, "128, 128, 2, 2, {}, 2, 1, 1", 32, True, "F32_GLDS F32_SPLIT_BF16", False, 130, 512, twin=12),
    _GatherTile("EMU", 17, 128, 64, "128, 64, 2, 1, {}, 3, 2, 1", 32, True, "F32_GLDS F32_SPLIT_BF16", False, 132, 512, twin=13),
    _GatherTile("EMU", 18, 64, 64, "64, 64, 2, 1, {}, 4, 2, 1", 32, True, "F32_GLDS F32_SPLIT_BF16", False, 134, 512, twin=14),
    _GatherTile("EMU", 19, 256, 128, "256, 128, 4, 2, {}, 3, 1, 1", 32, True, "F32_GLDS F32_SPLIT_BF16", False, 136, 256, twin=15),
)
_BF16_GATHER_TILES = (
    _GatherTile("HREG", 0, 128, 128, "128, 128, 2, 2, {}", 1, False, "", True, 60, 768),
    _GatherTile("HREG", 1, 256, 64, "256, 64, 4, 1, {}", 1, False, "", True, 63, 768),
    _GatherTile("HREG", 2, 64, 64, "64, 64, 2, 2, {}", 1, False, "", True, 66, 768),
    _GatherTile("HREG", 3, 256, 128, "256, 128, 4, 2, {}", 1, False, "", True, 69, 512),
    _GatherTile("HREG", 4, 128, 64, "128, 64, 4, 1, {}", 1, False, "", True, 72, 768),
    # 5..11: the LDS-DMA family (csrc/conv_gemm_bf16_glds.inc); with BN -> ReLU on load: the two-buffer tiles and the four-buffer
    # small one.  8 spills registers: not built, never offered
    _GatherTile("HGLDS", 5, 128, 128, "128, 128, 2, 2, {}, 2", 64, False, "BF16_GLDS", True, 80, 512, kind_bn=94),
    _GatherTile("HGLDS", 6, 128, 128, "128, 128, 2, 2, {}, 3", 64, False, "BF16_GLDS", False, 82, 256),
    _GatherTile("HGLDS", 7, 256, 128, "256, 128, 4, 2, {}, 2", 64, False, "BF16_GLDS", True, 84, 256, kind_bn=95),
    _GatherTile("HNONE", 8, 256, 128, "256, 128, 4, 2, {}, 3", 64, False, "BF16_GLDS", False, 86, None),
    _GatherTile("HGLDS", 9, 128, 64, "128, 64, 4, 1, {}, 2", 64, False, "BF16_GLDS", True, 88, 768, kind_bn=96),
    _GatherTile("HGLDS", 10, 128, 64, "128, 64, 4, 1, {}, 3", 64, False, "BF16_GLDS", False, 90, 512),
    _GatherTile("HGLDS", 11, 64, 64, "64, 64, 2, 2, {}, 4", 64, False, "BF16_GLDS", True, 92, 512, kind_bn=98),
)
_GATHER_KERNELS = {"LDS_S": "gather_gemm_kernel", "LDS": "gather_gemm_kernel", "DIRECT": "direct_gemm_kernel",
                   "GLDS": "gather_gemm_f32_glds_kernel", "EMU": "gather_gemm_f32_glds_kernel",
                   "HREG": "gather_gemm_bf16_kernel", "HGLDS": "gather_gemm_bf16_glds_kernel"}

# Weight gradients.  route: WgradRoute of the header (W_FOUR: 64 gathered channels x T channels of the small-grid operand).
#   targs    template arguments of the instantiations with the kinds kind, kind + 1, ..., in the order of the `switch` that ends
#            decide_wgrad: fp32 W_REG spec 0 / 1 / 2 (scalar_targs: kind 42 / 43), W_FOUR conv / transposed conv; W_MERGE the same;
#            else plain / BN -> ReLU on x.  The bf16 kinds do not distinguish POW2 (small grid a power of two: the argument after
#            the BN flag, W_FOUR's last): the name is the power-of-two instantiation's, or carries * for both
#   targets  blocks in flight the split candidates aim at; one_round: first, the largest split that fits ONE round of
#            tuner_resident blocks (one block per CU is usually the best -- rb2 of config #2, 24 channel-tile x class blocks:
#            split 10 = 240 blocks 92 us, split 8 = 192 blocks 105, split 11 = 264 blocks 148)
_PIXEL_TARGETS = (256, 512, 768, 1024, 1536, 2048, 4096)
_WgradTile = namedtuple("_WgradTile", "route id T kernel targs vec_only switches bn_form kind tuner_resident targets "
                                      "one_round scalar_targs twin", defaults=(_PIXEL_TARGETS, False, None, None))
_F32_WGRAD_TILES = (
    _WgradTile("W_REG", 0, 128, "wgrad_gemm_kernel", ("128, 128, true, 0", "128, 128, true, 1", "128, 128, true, 2"), False, "", True, 36, 768,
               scalar_targs="128, 128, false, 0"),
    _WgradTile("W_REG", 2, 64, "wgrad_gemm_kernel", ("64, 64, true, 0", "64, 64, true, 1", "64, 64, true, 2"), False, "", True, 39, 768,
               scalar_targs="64, 64, false, 0"),
    # 5 / 6 = the 128 / 64 tiles on LDS-DMA (csrc/conv_gemm_glds.inc); 7 / 8 = the same with the products on the bf16 matrix pipe
    _WgradTile("W_GLDS", 5, 128, "wgrad_gemm_f32_glds_kernel", ("128, false, 2, 0", "128, true, 2, 0"), True, "F32_GLDS", True, 116, 768),
    _WgradTile("W_GLDS", 6, 64, "wgrad_gemm_f32_glds_kernel", ("64, false, 4, 0", "64, true, 2, 0"), True, "F32_GLDS", True, 118, 768),
    _WgradTile("W_EMU", 7, 128, "wgrad_gemm_f32_glds_kernel", ("128, false, 2, 1",), True, "F32_GLDS F32_SPLIT_BF16", False, 138, 768, twin=5),
    _WgradTile("W_EMU", 8, 64, "wgrad_gemm_f32_glds_kernel", ("64, false, 4, 1",), True, "F32_GLDS F32_SPLIT_BF16", False, 139, 768, twin=6),
    # 9 / 10 (k4 s2 p1, small grid of whole 8 x 8 tiles): four taps -- one parity class -- per block, products on the bf16 matrix
    # pipe (csrc/conv_gemm_glds_parity.inc); without that pipe a plan on them runs on the 64 x 64 register-staged tile
    _WgradTile("W_FOUR", 9, 64, "wgrad_parity_f32_kernel", ("64, true", "64, false"), True, "F32_GLDS F32_SPLIT_BF16", False, 140, 256,
               (64, 128, 192, 256, 384, 512, 1024), True, twin=2),
    _WgradTile("W_FOUR", 10, 128, "wgrad_parity_f32_kernel", ("128, true", "128, false"), True, "F32_GLDS F32_SPLIT_BF16", False, 142, 256,
               (64, 128, 192, 256, 384, 512, 1024), True, twin=2),
)
_BF16_WGRAD_TILES = (
    _WgradTile("W_REG", 0, 128, "wgrad_gemm_bf16_kernel", ("128, 128, false, true", "128, 128, true, true"), False, "", True, 75, 768),
    _WgradTile("W_REG", 2, 64, "wgrad_gemm_bf16_kernel", ("64, 64, false, true", "64, 64, true, true"), False, "", True, 77, 768),
    _WgradTile("W_GLDS", 5, 128, "wgrad_gemm_bf16_glds_kernel", ("128, false, true, 0", "128, true, true, 0"), False, "BF16_GLDS", True, 100, 768),
    _WgradTile("W_GLDS", 6, 64, "wgrad_gemm_bf16_glds_kernel", ("64, false, true, 0", "64, true, true, 0"), False, "BF16_GLDS", True, 102, 768),
    # 7 (plain operand): two taps per block on the gathered operand's side when that side has 64 channels
    _WgradTile("W_MERGE", 7, 128, "wgrad_gemm_bf16_glds_kernel", ("128, false, true, 1", "128, false, true, 2"), False, "BF16_GLDS", False, 120, 768),
    # 8 / 9 (plain operand, k4 s2 p1, small grid of whole 8 x 8 tiles): four taps -- one parity class -- per block
    _WgradTile("W_FOUR", 8, 64, "wgrad_parity_bf16_kernel", ("64, *",), False, "BF16_GLDS WGRAD_PARITY", False, 122, 512, (256, 512, 768, 1024, 2048)),
    _WgradTile("W_FOUR", 9, 128, "wgrad_parity_bf16_kernel", ("128, *",), False, "BF16_GLDS WGRAD_PARITY", False, 123, 256, (256, 512, 768, 1024, 2048)),
)


def _tile_offered(t, g: "Geom", plain_operand: bool) -> bool:
    """what the tuner asks of any tile, gather or weight gradient: its switches on, a form for the operand, the vector path"""
    return (all(globals()[s] for s in t.switches.split()) and (t.bn_form or plain_operand)
            and not (t.vec_only and (g.Cin % 4 or g.Cout % 4)))


_forced_plan = None

# Committed launch plans: the tuner's choices for the BASELINE configurations, measured on an MI355X
# by tests/tools/make_plan_table.py and kept in mimic_amd/plans_gfx950.json.  A triple found in the table takes its plan
# from it; the tuner only runs for triples the table does not hold (other shapes / batch sizes), or for everything under
# MOPOE_AUTOTUNE=force.  Two processes therefore launch the same kernels, and a bench set-up does not spend its first
# step timing ~30 candidates per layer.
PLAN_TABLE_PATH = os.environ.get("MOPOE_PLAN_TABLE", os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans_gfx950.json"))
USE_PLAN_TABLE = os.environ.get("MOPOE_AUTOTUNE", "1") != "force" and os.environ.get("MOPOE_PLAN_TABLE", "") != "0"
_plan_table = None


def plan_key_str(key) -> str:
    """the table's key: op name, the 14 geometry numbers, the fusion flags"""
    g = key[1]
    geo = ",".join(str(int(getattr(g, f))) for f in ("N", "Hs", "Ws", "Hb", "Wb", "Cin", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "transposed"))
    return f"{key[0]}|{geo}|" + ",".join(str(int(f)) if isinstance(f, bool) else str(f) for f in key[2:])


def _table_plan(key):
    """(found, plan or None) from the committed table"""
    global _plan_table
    if _plan_table is None:
        _plan_table = {}
        if USE_PLAN_TABLE and os.path.exists(PLAN_TABLE_PATH):
            import json
            with open(PLAN_TABLE_PATH) as f:
                _plan_table = json.load(f).get("plans", {})
    v = _plan_table.get(plan_key_str(key), False)
    if v is False and key[0] in ("fwd", "fwd16") and len(key) >= 4 and isinstance(key[3], bool):
        # a forward conv with / without a dropout mask in its epilogue (train / eval, or dropout disabled): the table was measured
        # on the training step; the mask multiplies the finished tile and does not move the choice of tile or split
        v = _plan_table.get(plan_key_str(key[:3] + (not key[3],) + key[4:]), False)
    if v is False:
        return False, None
    if v is not None and not F32_SPLIT_BF16 and key[0] in ("fwd", "dgrad", "wgrad"):
        # the switch is off: a committed plan on the bf16 matrix pipe falls back to the tile's twin on the fp32 MFMA
        twin = next((t.twin for t in (_F32_WGRAD_TILES if key[0] == "wgrad" else _F32_GATHER_TILES) if t.id == v[0]), None)
        if twin is not None:
            v = [twin, v[1]]
    return True, (None if v is None else _Plan(int(v[0]), int(v[1])))


_plan_sources = {"table": 0, "tuned": 0, "static": 0}


def plan_source_summary():
    """how the launch plans in use were obtained: counts of (op, geometry, fusion) triples from the committed table, from the
    in-process tuner, and left on the library's static heuristic"""
    return dict(_plan_sources, table_file=os.path.basename(PLAN_TABLE_PATH) if USE_PLAN_TABLE and os.path.exists(PLAN_TABLE_PATH) else None)


def clear_plans():
    _plans.clear()


class force_plan:
    """context manager (tests): every conv op inside uses this (tile, split) instead of the tuned table"""

    def __init__(self, tile: int, split: int):
        self.plan = _Plan(tile, split)

    def __enter__(self):
        global _forced_plan
        self.prev, _forced_plan = _forced_plan, self.plan
        return self

    def __exit__(self, *exc):
        global _forced_plan
        _forced_plan = self.prev


_plan_log = {}


def plan_report():
    """[(op, geometry, fusion flags, chosen (tile, split), its us, {candidate: us})] of every tuned triple"""
    out = []
    for key, timings in _plan_log.items():
        p = _plans.get(key)
        chosen = None if p is None else (p.tile, p.split)
        out.append((key[0], key[1], key[2:], chosen, timings.get(chosen), timings))
    return out


def plan_table():
    """{(op, Geom, fusion flags): (tile, split) or None (static heuristic)} -- what the autotuner chose"""
    return {k: (None if v is None else (v.tile, v.split)) for k, v in _plans.items()}


def _gather_shape(kind: str, g: Geom):
    """(rows per phase, phases, taps per phase, K channels, N channels) of the implicit GEMM (conv_gemm.hip)"""
    ck, cn = (g.Cin, g.Cout) if kind == "fwd" else (g.Cout, g.Cin)
    dest_on_small = (kind == "fwd") != bool(g.transposed)
    if dest_on_small:
        return g.N * g.Hs * g.Ws, 1, g.kh * g.kw, ck, cn
    rows = g.N * -(-g.Hb // g.sh) * -(-g.Wb // g.sw)
    return rows, g.sh * g.sw, max(1, (g.kh // g.sh) * (g.kw // g.sw)), ck, cn


WS_COUNTER_BYTES = 64 << 10   # head of the workspace: arrival counters of in-kernel split reductions (header: workspace)


def _gather_tile_candidates(tiles, kind: str, g: Geom, ws_bytes: int, plain_operand: bool):
    """{(tile, split): fraction of the chip the launch occupies} of one family's table, in the order the tuner launches them"""
    bf16 = tiles is _BF16_GATHER_TILES
    ws_bytes -= WS_COUNTER_BYTES
    rows, nphase, taps, ck, cn = _gather_shape(kind, g)
    iters = taps * (ck // 32 if bf16 else -(-ck // 16))   # (the library's split policy counts 32- / 16-deep K steps)
    per = rows * nphase * cn * 4
    cands = {}
    for t in tiles:
        if t.kernel == "HNONE" or (t.bm == 256 and rows < 256) or ck % t.k_multiple or not _tile_offered(t, g, plain_operand):
            continue
        if t.kernel == "HGLDS" and taps * (ck // t.k_multiple) < 2:
            continue     # a single 64-deep chunk per tile: nothing to pipeline
        blocks = -(-rows // t.bm) * -(-cn // t.bn) * nphase
        cands[(t.id, 1)] = min(1.0, blocks / t.tuner_resident)
        for s in _SPLITS:
            if s * 2 <= iters and blocks * s <= 2048 and s * per <= ws_bytes:
                cands[(t.id, s)] = min(1.0, blocks * s / t.tuner_resident)
    return cands


def _gather_candidates(kind: str, g: Geom, ws_bytes: int, plain_operand: bool = False):
    """plain_operand: no BN -> ReLU on the gathered operand (every LDS-DMA tile applies; with it tiles 12, 14 and 15)"""
    if min(g.Cin, g.Cout) == 1:
        return {}   # image-side edge layers run on the streaming edge kernels: nothing to choose
    return _gather_tile_candidates(_F32_GATHER_TILES, kind, g, ws_bytes, plain_operand)


def _gather_candidates_bf16(kind: str, g: Geom, ws_bytes: int, plain_operand: bool = False):
    """plain_operand: the gathered operand enters the MFMA as it lies in memory (no BN -> ReLU on load): the LDS-DMA tiles apply"""
    return _gather_tile_candidates(_BF16_GATHER_TILES, kind, g, ws_bytes, plain_operand)


def _four_tap(g: Geom) -> bool:
    """k4 s2 p1 on a small grid of whole 8 x 8 tiles (conv_launch.hpp: four_tap_geometry)"""
    return ((g.kh, g.kw, g.sh, g.sw, g.ph, g.pw) == (4, 4, 2, 2, 1, 1) and g.Hs % 8 == 0 and g.Ws % 8 == 0
            and g.Hb == 2 * g.Hs and g.Wb == 2 * g.Ws)


def _offer_splits(cands, t, tiles: int, max_split: int):
    """the tile's targets -> distinct splits of the pixel reduction -> fraction of the chip each occupies"""
    for s in ([t.tuner_resident // tiles] if t.one_round else []) + [-(-target // tiles) for target in t.targets]:
        s = max(1, min(s, max_split))
        if (t.id, s) not in cands:
            cands[(t.id, s)] = min(1.0, tiles * s / t.tuner_resident)


def _wgrad_candidates(g: Geom, bf16: bool = False, plain_operand: bool = False):
    if min(g.Cin, g.Cout) == 1:
        return {}
    ms = g.N * g.Hs * g.Ws
    cg, csm = (g.Cout, g.Cin) if g.transposed else (g.Cin, g.Cout)   # channels of the gathered / the small-grid operand
    cands = {}
    # (the tuner launches candidates in insertion order: the routes with several taps per block first, as ever)
    for t in sorted(_BF16_WGRAD_TILES if bf16 else _F32_WGRAD_TILES, key=lambda t: t.route not in ("W_MERGE", "W_FOUR")):
        if not _tile_offered(t, g, plain_operand):
            continue
        if t.route == "W_MERGE":
            if g.taps % 2 == 0 and cg == 64:
                _offer_splits(cands, t, -(-csm // t.T) * (g.taps // 2), -(-ms // 128))
        elif t.route == "W_FOUR":
            if _four_tap(g) and csm % t.T == 0:
                _offer_splits(cands, t, -(-cg // 64) * (csm // t.T) * 4, g.N * (g.Hs // 8) * (g.Ws // 8))
        elif t.T == 64 or (g.Cin > 64 and g.Cout > 64):   # (a 128 tile would run half-empty MFMA tiles on <= 64 channels)
            _offer_splits(cands, t, -(-g.Cin // t.T) * -(-g.Cout // t.T) * g.taps, -(-ms // 128))
    return cands


_scratch = {}


def _scratch_like(t):
    """zero-initialised stand-in for an accumulating output while candidates are being timed"""
    if t is None:
        return None
    k = (t.dtype, t.numel(), t.device)
    if k not in _scratch:
        _scratch[k] = torch.zeros(t.numel(), dtype=t.dtype, device=t.device)
    return _scratch[k]


def _tuned_plan(key, cands_fn, launch):
    """launch(plan_ref) enqueues the op once on scratch accumulators -> ctypes byref of the fastest plan (or None)"""
    if _forced_plan is not None:
        return C.byref(_forced_plan)
    if key in _plans:
        p = _plans[key]
        return None if p is None else C.byref(p)
    if not AUTOTUNE and not TABLE_ONLY:
        return None
    found, p = _table_plan(key)
    if found:
        _plans[key] = p
        _plan_sources["table"] += 1
        return None if p is None else C.byref(p)
    if TABLE_ONLY and not AUTOTUNE:
        _plans[key] = None
        _plan_sources["static"] += 1
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    global _conv_calls
    _conv_calls += 1
    if _conv_calls <= TUNE_AFTER_CALLS:
        return None   # still warming up: static heuristic, nothing cached
    cands = cands_fn()
    best, timings = None, {}
    if len(cands) > 1:
        # candidates are timed alone on the device: work still queued on the other streams (the other modalities'
        # networks, the weight-gradient lane) would otherwise run beside them and decide the ranking
        torch.cuda.synchronize()
        def time_plan(plan, reps):
            ref = C.byref(plan)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch(ref)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3

        plans = {c: _Plan(*c) for c in cands}
        # objective: duration x (alpha + (1 - alpha) x fraction of the chip occupied).  alpha = 1 ranks by latency
        # alone; below 1 a launch that leaves CUs free for the other modalities' branches of the step graph is
        # charged less for its duration
        score = lambda c: timings[c] * (TUNE_ALPHA + (1.0 - TUNE_ALPHA) * cands[c])
        for c, plan in plans.items():          # pass 1: everything, briefly (first launch = warm-up)
            launch(C.byref(plan))
            timings[c] = time_plan(plan, _TUNE_REPS)
        finalists = sorted(timings, key=score)[:3]
        for c in finalists:                    # pass 2: the three best, longer; best of three batches each
            timings[c] = min(time_plan(plans[c], 2 * _TUNE_REPS) for _ in range(3))
        best = plans[min(finalists, key=score)]
    _plans[key] = best
    _plan_log[key] = timings
    _plan_sources["tuned" if len(cands) > 1 else "static"] += 1
    return None if best is None else C.byref(best)


BF16 = torch.bfloat16


def _is16(t):
    return t is not None and t.dtype == BF16


def conv_mix_supported(x, g: Geom) -> bool:
    """can conv_fwd(..., mix=) take this layer?  (the residual mix lives in the vector path's row-major epilogue)"""
    return _is16(x) or (g.Cin % 4 == 0 and g.Cout % 4 == 0)


def conv_fwd(x, wp, g: Geom, bn_in: Optional[Bn] = None, bias=None, mask: Optional[Mask] = None,
             out_stats=None, out_dtype=None, mix=None):
    """out_dtype: dtype of the result (default: the activation operand's).  bf16 family: x bf16 + wp bf16 (the
    weight copy); the single-channel image-side layers take the fp32 image / fp32 taps and a bf16 wide tensor.
    mix = (s, bn_s[, a, b]): the residual mix of a block in the epilogue, y = a * bn_s(s) + b * mask * (conv + bias)
    (include/mopoe_hip.h: mopoe_conv_fwd_mix); out_stats are then those of y."""
    _dev(x, wp, bias, out_stats)
    assert tuple(x.shape) == g.in_shape and tuple(wp.shape) == (g.taps, g.Cin, g.Cout)
    out_dtype = out_dtype or x.dtype
    gc = g.c()
    stream = _stream()
    mixr = None
    if mix is not None:
        ms, mbn = mix[0], mix[1]
        _dev(ms)
        assert tuple(ms.shape) == g.out_shape and ms.dtype == out_dtype and ms.is_contiguous() and conv_mix_supported(x, g)
        mixc = _MixRef(ms.data_ptr(), mbn.c(), float(mix[2]) if len(mix) > 2 else RES_A, float(mix[3]) if len(mix) > 3 else RES_B)
        mixr = C.byref(mixc)
    if _is16(x) or out_dtype == BF16:
        plain = bn_in is None and mask is None
        if not g.transposed and g.Cin == 1:      # image stem: fp32 pixels x fp32 taps -> bf16 features
            assert plain and bias is None and x.dtype == torch.float32 and wp.dtype == torch.float32
            y = torch.empty(g.out_shape, dtype=BF16, device=x.device)
            _check(lib().mopoe_edge_expand_bf16(_p(x), _p(wp), _p(y), C.byref(gc), g.Cout, _p(out_stats), stream))
            return y
        if g.transposed and g.Cout == 1:         # image head: bf16 features x fp32 taps -> fp32 pixels
            assert plain and out_stats is None and _is16(x) and wp.dtype == torch.float32
            y = torch.empty(g.out_shape, dtype=torch.float32, device=x.device)
            _check(lib().mopoe_edge_reduce_bf16(_p(x), _p(wp), _p(bias), _p(y), C.byref(gc), g.Cin, stream))
            return y
        if not (_is16(x) and _is16(wp)):
            raise MopoeHipError("bf16 conv needs a bf16 activation and the bf16 copy of the packed weight")
        y = torch.empty(g.out_shape, dtype=out_dtype, device=x.device)
        ws, nbytes = _workspace(x.device)
        fn = lib().mopoe_conv_fwd_bf16
        bnr, mr, f32 = _bn(bn_in), _mask(mask), C.c_int32(int(out_dtype == torch.float32))

        def launch16(plan, stats=None):
            if mixr is not None:
                _check(lib().mopoe_conv_fwd_mix_bf16(_p(x), _p(wp), _p(bias), _p(y), C.byref(gc), bnr, mr, mixr, _p(stats),
                                                     plan, _p(ws), C.c_size_t(nbytes), stream))
                return
            _check(fn(_p(x), _p(wp), _p(bias), _p(y), f32, C.byref(gc), bnr, mr, _p(stats), plan, _p(ws),
                      C.c_size_t(nbytes), stream))

        key = ("fwd16", g, bn_in is not None, mask is not None, out_stats is not None, out_dtype) + (("mix",) if mix is not None else ())
        plan = _tuned_plan(key, lambda: _gather_candidates_bf16("fwd", g, nbytes, plain_operand=bn_in is None),
                           lambda ref: launch16(ref, _scratch_like(out_stats)))
        launch16(plan, out_stats)
        return y
    y = torch.empty(g.out_shape, dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(x.device)
    fn = lib().mopoe_conv_fwd
    bnr, mr = _bn(bn_in), _mask(mask)

    def launch(plan, stats=None):
        if mixr is not None:
            _check(lib().mopoe_conv_fwd_mix(_p(x), _p(wp), _p(bias), _p(y), C.byref(gc), bnr, mr, mixr, _p(stats), plan,
                                            _p(ws), C.c_size_t(nbytes), stream))
            return
        _check(fn(_p(x), _p(wp), _p(bias), _p(y), C.byref(gc), bnr, mr, _p(stats), plan, _p(ws), C.c_size_t(nbytes),
                  stream))

    key = ("fwd", g, bn_in is not None, mask is not None, out_stats is not None) + (("mix",) if mix is not None else ())
    plan = _tuned_plan(key, lambda: _gather_candidates("fwd", g, nbytes, plain_operand=bn_in is None),
                       lambda ref: launch(ref, _scratch_like(out_stats)))
    launch(plan, out_stats)
    return y


def conv_dgrad(dy, wp, g: Geom, relu_bn: Optional[Bn] = None, xin=None, bwd_sums=None, out_dtype=None):
    _dev(dy, wp, xin, bwd_sums)
    assert tuple(dy.shape) == g.out_shape
    out_dtype = out_dtype or dy.dtype
    gc = g.c()
    stream = _stream()
    if _is16(dy) or out_dtype == BF16:
        if g.transposed and g.Cout == 1:         # image head: fp32 pixel gradient x fp32 taps -> bf16 feature gradient
            assert relu_bn is None and dy.dtype == torch.float32 and wp.dtype == torch.float32
            dx = torch.empty(g.in_shape, dtype=BF16, device=dy.device)
            _check(lib().mopoe_edge_expand_bf16(_p(dy), _p(wp), _p(dx), C.byref(gc), g.Cin, None, stream))
            return dx
        if not (_is16(dy) and _is16(wp)) or (xin is not None and not _is16(xin)):
            raise MopoeHipError("bf16 conv_dgrad needs bf16 dy / xin and the bf16 copy of the packed weight")
        dx = torch.empty(g.in_shape, dtype=out_dtype, device=dy.device)
        ws, nbytes = _workspace(dy.device)
        fn = lib().mopoe_conv_dgrad_bf16
        bnr, f32 = _bn(relu_bn), C.c_int32(int(out_dtype == torch.float32))

        def launch16(plan, sums=None):
            _check(fn(_p(dy), _p(wp), _p(dx), f32, C.byref(gc), bnr, _p(xin), _p(sums), plan, _p(ws), C.c_size_t(nbytes),
                      stream))

        key = ("dgrad16", g, relu_bn is not None, bwd_sums is not None, out_dtype)
        plan = _tuned_plan(key, lambda: _gather_candidates_bf16("dgrad", g, nbytes, plain_operand=True),
                           lambda ref: launch16(ref, _scratch_like(bwd_sums)))
        launch16(plan, bwd_sums)
        return dx
    dx = torch.empty(g.in_shape, dtype=torch.float32, device=dy.device)
    ws, nbytes = _workspace(dy.device)
    fn = lib().mopoe_conv_dgrad
    bnr = _bn(relu_bn)

    def launch(plan, sums=None):
        _check(fn(_p(dy), _p(wp), _p(dx), C.byref(gc), bnr, _p(xin), _p(sums), plan, _p(ws), C.c_size_t(nbytes), stream))

    key = ("dgrad", g, relu_bn is not None, bwd_sums is not None)
    plan = _tuned_plan(key, lambda: _gather_candidates("dgrad", g, nbytes, plain_operand=True),
                       lambda ref: launch(ref, _scratch_like(bwd_sums)))
    launch(plan, bwd_sums)
    return dx


def conv_wgrad(x, dy, g: Geom, bn_in: Optional[Bn] = None, out=None):
    """out: optional ZERO-FILLED [taps, Cin, Cout] destination (e.g. a slice of a per-network gradient arena).
    The result is fp32 for either family (it feeds Adam on the fp32 master weights)."""
    _dev(x, dy, out)
    assert tuple(x.shape) == g.in_shape and tuple(dy.shape) == g.out_shape
    dwp = out if out is not None else torch.empty((g.taps, g.Cin, g.Cout), dtype=torch.float32, device=x.device)
    assert tuple(dwp.shape) == (g.taps, g.Cin, g.Cout) and dwp.dtype == torch.float32
    gc = g.c()
    stream = _stream()
    bnr = _bn(bn_in)
    if _is16(x) or _is16(dy):
        if min(g.Cin, g.Cout) == 1:              # image stem / head: wide tensor bf16, image side fp32
            assert bn_in is None
            vec, scal = (dy, x) if g.Cin == 1 else (x, dy)
            assert _is16(vec) and scal.dtype == torch.float32
            _check(lib().mopoe_edge_wgrad_bf16(_p(vec), _p(scal), _p(dwp), C.byref(gc), max(g.Cin, g.Cout),
                                               C.c_int32(int(out is not None)), stream))
            return dwp
        if not (_is16(x) and _is16(dy)):
            raise MopoeHipError("bf16 conv_wgrad needs both operands in bf16")
        fn = lib().mopoe_conv_wgrad_bf16
        key = ("wgrad16", g, bn_in is not None)
    else:
        fn = lib().mopoe_conv_wgrad
        key = ("wgrad", g, bn_in is not None)

    def launch(plan, dst, is_zero):
        _check(fn(_p(x), _p(dy), _p(dst), C.byref(gc), bnr, C.c_int32(is_zero), plan, stream))

    plan = _tuned_plan(key, lambda: _wgrad_candidates(g, bf16=key[0] == "wgrad16", plain_operand=bn_in is None),
                       lambda ref: launch(ref, _scratch_like(dwp), 1))
    launch(plan, dwp, int(out is not None))
    return dwp


# ----------------------------------------------------------------------------------------------
# residual-block glue
# ----------------------------------------------------------------------------------------------
def _rows(t):
    return t.numel() // t.shape[-1]


def block_out_fwd(s, m, bn_s: Bn, a=RES_A, b=RES_B, out_stats=None):
    _dev(s, m, out_stats)
    out = torch.empty_like(s)
    fn = lib().mopoe_block_out_fwd_bf16 if _is16(s) else lib().mopoe_block_out_fwd
    _check(fn(_p(s), _p(m), _p(out), C.c_int64(_rows(s)), s.shape[-1], _bn(bn_s),
                                     C.c_float(a), C.c_float(b), _p(out_stats), _stream()))
    return out


def bn_relu_apply(x, bn: Bn):
    """relu(bn(x)) written out (the operand of a block's second conv, where that beats the conv's BN -> ReLU-on-load form)"""
    _dev(x)
    out = torch.empty_like(x)
    fn = lib().mopoe_bn_relu_apply_bf16 if _is16(x) else lib().mopoe_bn_relu_apply
    _check(fn(_p(x), _p(out), C.c_int64(_rows(x)), x.shape[-1], _bn(bn), _stream()))
    return out


# ---- the front of a residual block as streaming kernels (csrc/pointwise.hip): bn1 -> relu -> conv1 (1x1) -> dropout -> bn2 -> relu
BLOCK_FRONT = os.environ.get("MOPOE_BLOCK_FRONT", "1") != "0"     # A/B switch
BLOCK_FRONT_F32 = os.environ.get("MOPOE_BLOCK_FRONT_F32", "1") != "0"     # A/B switch for the fp32 family alone
# fp32: the two forward passes each pay conv1's 64 MFMAs per 32 pixels at the fp32 rate (one MFMA = 64 cycles for 2 k) and come
# out slower than conv_fwd + bn_relu_apply (rb1 at config #2: 101.9 against 91.7 us); the fused backward wins (100.0 against
# 129.9 us).  So the fp32 family keeps the forward of round 3 (d1 written) and takes only the backward kernel.
BLOCK_FRONT_F32_FWD = os.environ.get("MOPOE_BLOCK_FRONT_F32_FWD", "0") != "0"


def block_front_supported(x, g1: "Geom", mask1: Optional[Mask], forward: bool = False) -> bool:
    """64 channels (either storage family), a 1x1 conv, dropout absent or per (sample, channel) on whole 32-row tiles.
    forward=True: is the FORWARD pair (statistics + apply passes, d1 never written) to be used as well?"""
    if forward and not _is16(x) and not BLOCK_FRONT_F32_FWD:
        return False
    return (BLOCK_FRONT and x.dtype in (BF16, torch.float32) and (_is16(x) or BLOCK_FRONT_F32) and g1.Cin == 64 and g1.Cout == 64
            and g1.taps == 1 and _rows(x) % 32 == 0
            and (mask1 is None or (mask1.kind == 1 and mask1.rows_per_sample % 32 == 0)))


def block_front_stats(x, w1, bias, bn1: Bn, mask1: Optional[Mask], out_stats):
    """out_stats [2, C] += {sum, sumsq} of d1 = mask1 * (conv1(relu(bn1(x))) + bias), rounded to bf16; d1 itself is not written"""
    _dev(x, w1, bias, out_stats)
    fn = lib().mopoe_block_front_stats_bf16 if _is16(x) else lib().mopoe_block_front_stats
    _check(fn(_p(x), _p(w1), _p(bias), C.c_int64(_rows(x)), x.shape[-1], _bn(bn1), _mask(mask1),
                                              _p(out_stats), _stream()))
    return out_stats


def block_front_apply(x, w1, bias, bn1: Bn, bn2: Bn, mask1: Optional[Mask]):
    """a2 = relu(bn2(d1)) with d1 recomputed from x"""
    _dev(x, w1, bias)
    a2 = torch.empty_like(x)
    fn = lib().mopoe_block_front_apply_bf16 if _is16(x) else lib().mopoe_block_front_apply
    _check(fn(_p(x), _p(w1), _p(bias), _p(a2), C.c_int64(_rows(x)), x.shape[-1], _bn(bn1), _bn(bn2),
                                              _mask(mask1), _stream()))
    return a2


def block_front_bwd(x, dh2, w1, bias, bn1: Bn, bn2: Bn, mask1: Optional[Mask], sums2, sums1, dw1, dbias=None, dgamma2=None,
                    dbeta2=None):
    """dh2 (conv2's input gradient, ReLU mask of bn2 applied) + sums2 -> dh1 (returned), sums1 [2, C] +=, dw1 [1, C, C] +=,
    dbias [C] += (pre-zeroed accumulators); dgamma2 / dbeta2 [C] = bn2's affine gradients (= sums2[1] / sums2[0])"""
    _dev(x, dh2, w1, bias, sums2, sums1, dw1, dbias, dgamma2, dbeta2)
    dh1 = torch.empty_like(x)
    fn = lib().mopoe_block_front_bwd_bf16 if _is16(x) else lib().mopoe_block_front_bwd
    _check(fn(_p(x), _p(dh2), _p(w1), _p(bias), _p(dh1), C.c_int64(_rows(x)), x.shape[-1], _bn(bn1),
                                            _bn(bn2), _mask(mask1), _p(sums2), _p(sums1), _p(dw1), _p(dbias), _p(dgamma2), _p(dbeta2),
                                            _stream()))
    return dh1


def bn_bwd_reduce(g, s, bn_s: Bn, sums=None):
    """sums: optional pre-zeroed double [2, C] (callers batch these allocations)."""
    _dev(g, s, sums)
    if sums is None:
        sums = new_stats(s.shape[-1], s.device)
    fn = lib().mopoe_bn_bwd_reduce_bf16 if _is16(s) else lib().mopoe_bn_bwd_reduce
    _check(fn(_p(g), _p(s), C.c_int64(_rows(s)), s.shape[-1], _bn(bn_s), _p(sums), _stream()))
    return sums


def block_out_bwd(g, s, bn_s: Bn, sums, mask: Optional[Mask], a=RES_A, b=RES_B, want_colsum_dm=False,
                  want_colsum_ds=True, small=None):
    """-> dm, ds, dgamma_s, dbeta_s, colsum_dm (or None), colsum_ds (or None)
    small: optional pre-zeroed float [4, C] that receives dgamma, dbeta and the two column sums."""
    _dev(g, s, sums)
    c = s.shape[-1]
    dm, ds = torch.empty_like(g), torch.empty_like(g)
    if small is None:
        small = torch.zeros(4, c, dtype=torch.float32, device=g.device)
    cdm = small[2] if want_colsum_dm else None
    cds = small[3] if want_colsum_ds else None
    fn = lib().mopoe_block_out_bwd_bf16 if _is16(s) else lib().mopoe_block_out_bwd
    _check(fn(_p(g), _p(s), _p(dm), _p(ds), C.c_int64(_rows(s)), c, _bn(bn_s), _p(sums), _mask(mask), C.c_float(a),
              C.c_float(b), _p(small[0]), _p(small[1]), _p(cdm), _p(cds), _stream()))
    return dm, ds, small[0], small[1], cdm, cds


def bn_bwd_apply(dy, x, bn: Bn, sums, mask: Optional[Mask] = None, add=None, want_colsum=False, small=None,
                 next_s=None, next_bn: Optional[Bn] = None, next_sums=None):
    """-> dx, dgamma, dbeta, colsum_dx (or None); small: optional pre-zeroed float [3, C].
    next_s / next_bn / next_sums: also accumulate bn_bwd_reduce(dx, next_s, next_bn) into the pre-zeroed next_sums."""
    _dev(dy, x, sums, add, next_s, next_sums)
    c = x.shape[-1]
    dx = torch.empty_like(x)
    if small is None:
        small = torch.zeros(3, c, dtype=torch.float32, device=x.device)
    cs = small[2] if want_colsum else None
    nb = _bn(next_bn) if next_s is not None else None
    fn = lib().mopoe_bn_bwd_apply_bf16 if _is16(x) else lib().mopoe_bn_bwd_apply
    _check(fn(_p(dy), _p(x), _p(add), _p(dx), C.c_int64(_rows(x)), c, _bn(bn), _p(sums), _mask(mask), _p(small[0]),
              _p(small[1]), _p(cs), _p(next_s), nb, _p(next_sums), _stream()))
    return dx, small[0], small[1], cs


def bn_running_update(entries: Sequence, momentum=0.1):
    """entries: iterable of (sums double[2,C], running_mean, running_var, count).  One launch per 32 layers; the
    records travel in the kernel arguments, so there is no device-side table to build or keep alive."""
    entries = list(entries)
    if not entries:
        return
    arr = (_RunDesc * len(entries))()
    for i, (sums, rm, rv, count) in enumerate(entries):
        _dev(sums, rm, rv)
        arr[i] = _RunDesc(sums.data_ptr(), rm.data_ptr(), rv.data_ptr(), rm.numel(), count)
    _check(lib().mopoe_bn_running_update(arr, len(entries), C.c_float(momentum), _stream()))


# timeline stamps (tuning aid, tests/tools/net_timeline.py): when STAMPS is a dict, stamp(name) appends a device timestamp
# taken when the current stream reaches this point; the launches are captured like any other node of the step
STAMPS = None


def stamp(name):
    st = STAMPS
    if st is None:
        return
    if "buf" not in st:
        st["buf"] = torch.zeros(256, dtype=torch.int64, device="cuda")
        st["names"] = []
    i = len(st["names"])
    if i >= st["buf"].numel():
        return
    st["names"].append(name)
    _check(lib().mopoe_prof_stamp(C.c_void_p(st["buf"].data_ptr() + 8 * i), _stream()))


CLIP_NORM, CLIP_SCALE, CLIP_SKIP, CLIP_SKIPPED_TOTAL, CLIP_STATE_LEN = 0, 1, 2, 3, 4   # include/mopoe_hip_optim.h: the clip state
GRAD_NORM_CHUNK = 4096     # elements per partial sum (csrc/adam.hip: ADAM_CHUNK)


def grad_norm_partials(numels) -> int:
    """doubles of scratch that suffice for grad_norm over tensors of these sizes, whichever of them have a gradient
    (header: mopoe_grad_norm_partials)"""
    n = len(numels)
    arr = (_AdamSeg * n)()
    for i, k in enumerate(numels):
        arr[i] = _AdamSeg(None, None, None, None, None, int(k))
    fn = lib().mopoe_grad_norm_partials
    fn.restype = C.c_int64
    count = int(fn(arr, n))
    if count < 0:
        _check(count)
    return count


def grad_norm(grads, max_norm, state, scratch):
    """The global L2 norm of all gradients and the clip decision it implies (header: mopoe_grad_norm), deterministic and
    without a host sync.  grads: list of fp32 tensors (None entries contribute nothing); state: float32 [4] on the device,
    left as {norm before clipping, scale = min(1, max_norm / (norm + 1e-6)), skip (1 if the norm is not finite),
    skipped_total += skip}; scratch: float64 [>= grad_norm_partials(sizes)].  Returns state (adam_step's clip=)."""
    if state.dtype != torch.float32 or state.numel() != CLIP_STATE_LEN or scratch.dtype != torch.float64:
        raise MopoeHipError("grad_norm: state is float32 [4], scratch is float64")
    _dev(state, scratch)
    n = len(grads)
    arr = (_AdamSeg * n)()
    for i, g_ in enumerate(grads):
        if g_ is None:
            arr[i] = _AdamSeg(None, None, None, None, None, 0)
            continue
        if g_.dtype != torch.float32:
            raise MopoeHipError("grad_norm: gradients must be fp32 tensors")
        _dev(g_)
        arr[i] = _AdamSeg(None, g_.data_ptr(), None, None, None, g_.numel())
    _check(lib().mopoe_grad_norm(arr, n, C.c_double(float(max_norm)), _p(scratch), C.c_int64(scratch.numel()), _p(state),
                                 _stream()))
    return state


def adam_step(params, grads, ms, vs, step, lr, beta1, beta2, eps, coef, lowp=None, prep=True, clip=None):
    """One Adam step over all tensors (header: mopoe_adam_step).  params / grads / ms / vs: equally long lists of fp32
    tensors (a grad may be None: that tensor is skipped, like optim.Adam does); step: device scalar (float), incremented;
    lr: float or device scalar; coef: float[2] device scratch; lowp: optional list of bf16 copies (or None entries)
    rewritten in the same pass.  clip: the state grad_norm left (header: mopoe_adam_step_clipped): every gradient is
    multiplied by its scale as it is loaded, and nothing at all is written -- step and coef included -- when it says skip."""
    n = len(params)
    arr = (_AdamSeg * n)()
    for i in range(n):
        p_, g_ = params[i], grads[i]
        if g_ is None:
            arr[i] = _AdamSeg(p_.data_ptr(), None, ms[i].data_ptr(), vs[i].data_ptr(), None, p_.numel())
            continue
        if g_.dtype != torch.float32 or p_.dtype != torch.float32 or g_.numel() != p_.numel():
            raise MopoeHipError("adam_step: parameters and gradients must be fp32 tensors of equal size")
        _dev(p_, g_, ms[i], vs[i])
        lp = lowp[i] if lowp is not None else None
        arr[i] = _AdamSeg(p_.data_ptr(), g_.data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(),
                          None if lp is None else lp.data_ptr(), p_.numel())
    lr_dev = lr if isinstance(lr, torch.Tensor) else None
    if clip is not None:
        if clip.dtype != torch.float32 or clip.numel() != CLIP_STATE_LEN:
            raise MopoeHipError("adam_step: clip is the float32 [4] state of grad_norm")
        _dev(clip)
        _check(lib().mopoe_adam_step_clipped(arr, n, _p(step) if prep else None, _p(lr_dev),
                                             C.c_double(0.0 if lr_dev is not None else float(lr)), C.c_double(beta1),
                                             C.c_double(beta2), C.c_double(eps), _p(coef), _p(clip), _stream()))
        return
    _check(lib().mopoe_adam_step(arr, n, _p(step) if prep else None, _p(lr_dev), C.c_double(0.0 if lr_dev is not None else float(lr)),
                                 C.c_double(beta1), C.c_double(beta2), C.c_double(eps), _p(coef), _stream()))


def _ema_records(who, params, emas, lowp=None):
    n = len(params)
    arr = (_EmaSeg * n)()
    for i in range(n):
        p_, e_ = params[i], emas[i]
        if p_.dtype != torch.float32 or e_.dtype != torch.float32 or e_.numel() != p_.numel():
            raise MopoeHipError(f"{who}: parameters and averages must be fp32 tensors of equal size")
        lp = lowp[i] if lowp is not None else None
        if lp is not None and (lp.dtype != torch.bfloat16 or lp.numel() != p_.numel()):
            raise MopoeHipError(f"{who}: a low-precision copy must be a bf16 tensor of its parameter's size")
        _dev(p_, e_, lp)
        arr[i] = _EmaSeg(p_.data_ptr(), e_.data_ptr(), None if lp is None else lp.data_ptr(), p_.numel())
    return arr, n


def ema_update(params, emas, decay, step, clip=None):
    """ema += w * (p - ema) over all tensors (header: mopoe_ema_update), w = 1 - min(decay, (1 + step) / (10 + step)) formed
    on the device from `step`, Adam's device step counter after this step's increment.  params / emas: equally long lists
    of fp32 tensors; clip: the state grad_norm left -- nothing at all is written when it says the step was skipped."""
    arr, n = _ema_records("ema_update", params, emas)
    if step.dtype != torch.float32:
        raise MopoeHipError("ema_update: step is Adam's float32 device step counter")
    _dev(step)
    if clip is not None:
        if clip.dtype != torch.float32 or clip.numel() != CLIP_STATE_LEN:
            raise MopoeHipError("ema_update: clip is the float32 [4] state of grad_norm")
        _dev(clip)
    _check(lib().mopoe_ema_update(arr, n, C.c_double(float(decay)), _p(step), _p(clip), _stream()))


def ema_swap(params, emas, lowp=None):
    """Exchange every parameter with its average in place, bit for bit (header: mopoe_ema_swap); lowp: optional list of
    bf16 copies (or None entries), rewritten from the values the parameters then hold."""
    arr, n = _ema_records("ema_swap", params, emas, lowp)
    _check(lib().mopoe_ema_swap(arr, n, _stream()))


def colsum(x, out=None):
    """out: optional ZERO-FILLED [C] fp32 destination (a slice of a per-network gradient arena: no memset node)"""
    _dev(x, out)
    zero = out is not None
    if out is None:
        out = torch.empty(x.shape[-1], dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.numel() == x.shape[-1]
    fn = lib().mopoe_colsum_bf16 if _is16(x) else lib().mopoe_colsum
    _check(fn(_p(x), _p(out), C.c_int64(_rows(x)), x.shape[-1], C.c_int32(int(zero)), _stream()))
    return out


# ----------------------------------------------------------------------------------------------
# latent space
# ----------------------------------------------------------------------------------------------
def _ptr3(ts):
    arr = (C.c_void_p * 3)()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


_kl_ws = {}


def _ws(device, n=8):
    key = (device.index, n, _stream_ptr(device) if device.type == "cuda" else 0)
    if key not in _kl_ws:
        _kl_ws[key] = torch.zeros(n, dtype=torch.float64, device=device)
    return _kl_ws[key]


def latent_fwd(mu_in, lv_in, eps, row_start, w, norm):
    """mu_in/lv_in: 3-lists (PA, Lateral, text) of [B,D] or None.
    -> mus [K,B,D], lvs [K,B,D], joint_mu, joint_lv, z, klds [K], joint_div [1]"""
    present = [t for t in mu_in if t is not None]
    _dev(*present, *[t for t in lv_in if t is not None], eps)
    b, d = present[0].shape
    k = len(row_start) - 1
    dev = present[0].device
    mus = torch.empty(k, b, d, dtype=torch.float32, device=dev)
    lvs = torch.empty_like(mus)
    jm, jl, z = (torch.empty(b, d, dtype=torch.float32, device=dev) for _ in range(3))
    klds = torch.empty(k, dtype=torch.float32, device=dev)
    jd = torch.empty(1, dtype=torch.float32, device=dev)
    rs = (C.c_int32 * (k + 1))(*row_start)
    wa = (C.c_float * k)(*w)
    _check(lib().mopoe_latent_fwd(_ptr3(mu_in), _ptr3(lv_in), _p(eps), b, d, rs, wa, C.c_float(norm), _p(mus),
                                  _p(lvs), _p(jm), _p(jl), _p(z), _p(klds), _p(jd), _p(_ws(dev)),
                                  _stream()))
    return mus, lvs, jm, jl, z, klds, jd


def latent_bwd(mu_in, lv_in, eps, row_start, w, norm, g_mus, g_lvs, g_jm, g_jl, g_z, g_klds, g_jd):
    """-> (d_mu_in[3], d_lv_in[3]) with None for absent modalities."""
    present = [t for t in mu_in if t is not None]
    _dev(*present, eps, *[t for t in (g_mus, g_lvs, g_jm, g_jl, g_z, g_klds, g_jd) if t is not None])
    b, d = present[0].shape
    dmu = [None if t is None else torch.empty_like(t) for t in mu_in]
    dlv = [None if t is None else torch.empty_like(t) for t in lv_in]
    k = len(row_start) - 1
    rs = (C.c_int32 * (k + 1))(*row_start)
    wa = (C.c_float * k)(*w)
    _check(lib().mopoe_latent_bwd(_ptr3(mu_in), _ptr3(lv_in), _p(eps), b, d, rs, wa, C.c_float(norm), _p(g_mus),
                                  _p(g_lvs), _p(g_jm), _p(g_jl), _p(g_z), _p(g_klds), _p(g_jd), _ptr3(dmu),
                                  _ptr3(dlv), _stream()))
    return dmu, dlv


LATENT_METHODS = {"moe": 0, "jsd": 1}   # MOPOE_LATENT_MOE / MOPOE_LATENT_JSD


def _mixture_args(method, mu_in, member_row_start, comp_row_start, w):
    if method not in LATENT_METHODS:
        raise MopoeHipError(f"latent_mixture: method must be one of {sorted(LATENT_METHODS)}, not {method!r}")
    n = sum(t is not None for t in mu_in)
    c = n + (method == "jsd")
    if len(comp_row_start) != c + 1 or len(w) != c:
        raise MopoeHipError(f"latent_mixture: {method} with {n} modalities takes {c} components")
    flat = [v for part in member_row_start for v in (list(part) + [0] * 4)[:4]]
    if len(flat) != 12:
        raise MopoeHipError("latent_mixture: member_row_start holds the partitions over 1, 2 and 3 members")
    return (LATENT_METHODS[method], c, (C.c_int32 * 12)(*flat), (C.c_int32 * (c + 1))(*comp_row_start),
            (C.c_float * c)(*w))


def latent_mixture_fwd(method, mu_in, lv_in, eps, member_row_start, comp_row_start, w, norm):
    """method 'moe' or 'jsd'; mu_in/lv_in: 3-lists (PA, Lateral, text) of [B,D] or None; member_row_start: the row
    partitions over 1, 2 and 3 subset members; comp_row_start [C+1] / w [C]: the joint's partition over the C components
    and the joint divergence weights.
    -> sub_mu, sub_lv [K,B,D], comp_mu, comp_lv [C,B,D], joint_mu, joint_lv, z, klds [K], individual_divs [C],
       joint_div [1], pd_mu, pd_lv (jsd; None for moe)"""
    present = [t for t in mu_in if t is not None]
    _dev(*present, *[t for t in lv_in if t is not None], eps)
    b, d = present[0].shape
    m, c, mrs, crs, wa = _mixture_args(method, mu_in, member_row_start, comp_row_start, w)
    k = (1 << len(present)) - 1
    dev = present[0].device
    sub_mu = torch.empty(k, b, d, dtype=torch.float32, device=dev)
    sub_lv = torch.empty_like(sub_mu)
    comp_mu = torch.empty(c, b, d, dtype=torch.float32, device=dev)
    comp_lv = torch.empty_like(comp_mu)
    jm, jl, z = (torch.empty(b, d, dtype=torch.float32, device=dev) for _ in range(3))
    klds = torch.empty(k, dtype=torch.float32, device=dev)
    indiv = torch.empty(c, dtype=torch.float32, device=dev)
    jd = torch.empty(1, dtype=torch.float32, device=dev)
    pd_mu, pd_lv = (torch.empty(b, d, dtype=torch.float32, device=dev) for _ in range(2)) if method == "jsd" \
        else (None, None)
    _check(lib().mopoe_latent_mixture_fwd(m, _ptr3(mu_in), _ptr3(lv_in), _p(eps), b, d, mrs, crs, wa, C.c_float(norm),
                                          _p(sub_mu), _p(sub_lv), _p(comp_mu), _p(comp_lv), _p(jm), _p(jl), _p(z),
                                          _p(klds), _p(indiv), _p(jd), _p(pd_mu), _p(pd_lv), _p(_ws(dev, 16)),
                                          _stream()))
    return sub_mu, sub_lv, comp_mu, comp_lv, jm, jl, z, klds, indiv, jd, pd_mu, pd_lv


def latent_mixture_bwd(method, mu_in, lv_in, eps, member_row_start, comp_row_start, w, norm, g_sub_mu, g_sub_lv,
                       g_comp_mu, g_comp_lv, g_jm, g_jl, g_z, g_klds, g_indiv, g_jd, g_pd_mu=None, g_pd_lv=None):
    """-> (d_mu_in[3], d_lv_in[3]) with None for absent modalities; every g_* may be None."""
    gs = (g_sub_mu, g_sub_lv, g_comp_mu, g_comp_lv, g_jm, g_jl, g_z, g_klds, g_indiv, g_jd, g_pd_mu, g_pd_lv)
    present = [t for t in mu_in if t is not None]
    _dev(*present, eps, *[t for t in gs if t is not None])
    b, d = present[0].shape
    m, _c, mrs, crs, wa = _mixture_args(method, mu_in, member_row_start, comp_row_start, w)
    dmu = [None if t is None else torch.empty_like(t) for t in mu_in]
    dlv = [None if t is None else torch.empty_like(t) for t in lv_in]
    _check(lib().mopoe_latent_mixture_bwd(m, _ptr3(mu_in), _ptr3(lv_in), _p(eps), b, d, mrs, crs, wa, C.c_float(norm),
                                          *[_p(t) for t in gs], _ptr3(dmu), _ptr3(dlv), _stream()))
    return dmu, dlv


def _style_args(smu, slv, eps_s):
    present = [m for m in range(3) if smu[m] is not None]
    if not present:
        raise MopoeHipError("latent_style: no modality present")
    for m in range(3):
        if (smu[m] is None) != (slv[m] is None) or (smu[m] is None) != (eps_s[m] is None):
            raise MopoeHipError(f"latent_style: slot {m}: mu / logvar / eps presence mismatch")
    b = smu[present[0]].shape[0]
    s = [0 if smu[m] is None else smu[m].shape[1] for m in range(3)]
    for m in present:
        if smu[m].dim() != 2 or smu[m].shape[0] != b or slv[m].shape != smu[m].shape or eps_s[m].shape != smu[m].shape:
            raise MopoeHipError(f"latent_style: slot {m}: mu, logvar and eps must all be [B, S]")
    return present, b, s, (C.c_int32 * 3)(*s)


def latent_style_fwd(smu, slv, eps_s, z, norm):
    """style stage after the content latent kernel.  smu/slv/eps_s: 3-lists (PA, Lateral, text) of [B,S_m] or None;
    z [B,D] the content sample.
    -> zcat (3-list of [B, S_m + D] = [z_style_m | z], None for absent modalities), klds_style [3]"""
    present, b, s, sa = _style_args(smu, slv, eps_s)
    _dev(*[t for ts in (smu, slv, eps_s) for t in ts if t is not None], z)
    if z.dim() != 2 or z.shape[0] != b:
        raise MopoeHipError("latent_style_fwd: z must be [B, D]")
    d = z.shape[1]
    zcat = [None if smu[m] is None else torch.empty(b, s[m] + d, dtype=torch.float32, device=z.device) for m in range(3)]
    klds = torch.empty(3, dtype=torch.float32, device=z.device)
    _check(lib().mopoe_latent_style_fwd(_ptr3(smu), _ptr3(slv), _ptr3(eps_s), sa, b, d, _p(z), C.c_float(norm),
                                        _ptr3(zcat), _p(klds), _p(_ws(z.device, 4)), _stream()))
    return zcat, klds


def latent_style_bwd(smu, slv, eps_s, d, norm, g_zcat, g_klds):
    """g_zcat: 3-list of [B, S_m + D] or None (or None); g_klds [3] or None.
    -> (d_smu[3], d_slv[3]) with None for absent modalities, g_z [B, D]"""
    present, b, s, sa = _style_args(smu, slv, eps_s)
    g_zcat = list(g_zcat) if g_zcat is not None else [None] * 3
    for m in range(3):
        if g_zcat[m] is not None and (smu[m] is None or tuple(g_zcat[m].shape) != (b, s[m] + d)):
            raise MopoeHipError(f"latent_style_bwd: slot {m}: g_zcat must be [B, S + D] of a present modality")
    _dev(*[t for ts in (smu, slv, eps_s, g_zcat) for t in ts if t is not None], g_klds)
    dev = smu[present[0]].device
    dmu = [None if t is None else torch.empty_like(t) for t in smu]
    dlv = [None if t is None else torch.empty_like(t) for t in slv]
    g_z = torch.empty(b, d, dtype=torch.float32, device=dev)
    _check(lib().mopoe_latent_style_bwd(_ptr3(smu), _ptr3(slv), _ptr3(eps_s), sa, b, d, C.c_float(norm), _ptr3(g_zcat),
                                        _p(g_klds), _ptr3(dmu), _ptr3(dlv), _p(g_z), _stream()))
    return dmu, dlv, g_z


# ----------------------------------------------------------------------------------------------
# likelihoods, embedding
# ----------------------------------------------------------------------------------------------
def laplace_nll_fwd(x_hat, x, scale, norm):
    _dev(x_hat, x)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _check(lib().mopoe_laplace_nll_fwd(_p(x_hat), _p(x), C.c_int64(x.numel()), C.c_float(scale), C.c_float(norm),
                                       _p(out), _p(_ws(x.device)), _stream()))
    return out


def laplace_nll_bwd(x_hat, x, g, scale, norm):
    _dev(x_hat, x, g)
    dx = torch.empty_like(x_hat)
    _check(lib().mopoe_laplace_nll_bwd(_p(x_hat), _p(x), _p(g), C.c_int64(x.numel()), C.c_float(scale),
                                       C.c_float(norm), _p(dx), _stream()))
    return dx


def logsoftmax_fwd(x, inplace=False):
    _dev(x)
    y = x if inplace else torch.empty_like(x)
    _check(lib().mopoe_logsoftmax_fwd(_p(x), _p(y), C.c_int64(_rows(x)), x.shape[-1], _stream()))
    return y


def logsoftmax_bwd(dy, y, inplace=False, out_dtype=None):
    """out_dtype=bfloat16: the gradient of the logits leaves as a bf16 GEMM operand (dy, y are fp32)"""
    _dev(dy, y)
    if out_dtype == BF16:
        dx = torch.empty(dy.shape, dtype=BF16, device=dy.device)
        _check(lib().mopoe_logsoftmax_bwd_bf16out(_p(dy), _p(y), _p(dx), C.c_int64(_rows(y)), y.shape[-1], _stream()))
        return dx
    dx = dy if inplace else torch.empty_like(dy)
    _check(lib().mopoe_logsoftmax_bwd(_p(dy), _p(y), _p(dx), C.c_int64(_rows(y)), y.shape[-1], _stream()))
    return dx


def token_softmax_grad(logp, ids, g, norm, out_dtype=None):
    """gradient of the logits for loss = -sum_r logp[r, ids[r]] / norm with upstream gradient g (1 element), one pass"""
    _dev(logp, ids, g)
    out_dtype = out_dtype or torch.float32
    dx = torch.empty(logp.shape, dtype=out_dtype, device=logp.device)
    _check(lib().mopoe_token_softmax_grad(_p(logp), _p(ids), _p(g), C.c_int64(ids.numel()), logp.shape[-1], C.c_float(norm),
                                          _p(dx), C.c_int32(int(out_dtype == BF16)), _stream()))
    return dx


def lse_rows(logits):
    """logits [..., V] (fp32 or bf16, contiguous, V a multiple of 4 / 8) -> log-sum-exp per row, fp32 [...]"""
    _dev(logits)
    assert logits.is_contiguous()
    lse = torch.empty(logits.shape[:-1], dtype=torch.float32, device=logits.device)
    _check(lib().mopoe_lse_rows(_p(logits), C.c_int32(int(logits.dtype == BF16)), C.c_int64(_rows(logits)), logits.shape[-1],
                                _p(lse), _stream()))
    return lse


def token_nll_logits_fwd(logits, lse, ids, norm):
    """sum_r (lse[r] - logits[r, ids[r]]) / norm: the token NLL from the head's logits and their row log-sum-exp"""
    _dev(logits, lse, ids)
    out = torch.empty(1, dtype=torch.float32, device=logits.device)
    _check(lib().mopoe_token_nll_logits_fwd(_p(logits), C.c_int32(int(logits.dtype == BF16)), _p(lse), _p(ids),
                                            C.c_int64(ids.numel()), logits.shape[-1], C.c_float(norm), _p(out),
                                            _p(_ws(logits.device)), _stream()))
    return out


def token_softmax_grad_logits(logits, lse, ids, g, norm, inplace=False):
    """gradient of the logits for the token NLL from the logits themselves: g / norm * (softmax - onehot), in logits' dtype"""
    _dev(logits, lse, ids, g)
    dx = logits if inplace else torch.empty_like(logits)
    _check(lib().mopoe_token_softmax_grad_logits(_p(logits), C.c_int32(int(logits.dtype == BF16)), _p(lse), _p(ids), _p(g),
                                                 C.c_int64(ids.numel()), logits.shape[-1], C.c_float(norm), _p(dx), _stream()))
    return dx


def token_nll_fwd(logp, ids, norm):
    _dev(logp, ids)
    out = torch.empty(1, dtype=torch.float32, device=logp.device)
    _check(lib().mopoe_token_nll_fwd(_p(logp), _p(ids), C.c_int64(ids.numel()), logp.shape[-1], C.c_float(norm),
                                     _p(out), _p(_ws(logp.device)), _stream()))
    return out


def token_nll_bwd(ids, g, shape, norm):
    _dev(ids, g)
    dlogp = torch.empty(shape, dtype=torch.float32, device=ids.device)
    _check(lib().mopoe_token_nll_bwd(_p(ids), _p(g), C.c_int64(ids.numel()), shape[-1], C.c_float(norm),
                                     _p(dlogp), _stream()))
    return dlogp


def dense_nll_fwd(logp, target, norm):
    """-sum(target * logp) / norm (char text encoding: dense / one-hot targets)"""
    _dev(logp, target)
    assert logp.shape == target.shape
    out = torch.empty(1, dtype=torch.float32, device=logp.device)
    _check(lib().mopoe_dense_nll_fwd(_p(logp), _p(target), C.c_int64(logp.numel()), C.c_float(norm), _p(out),
                                     _p(_ws(logp.device)), _stream()))
    return out


def dense_nll_bwd(target, g, norm):
    _dev(target, g)
    dlogp = torch.empty_like(target)
    _check(lib().mopoe_dense_nll_bwd(_p(target), _p(g), C.c_int64(target.numel()), C.c_float(norm), _p(dlogp), _stream()))
    return dlogp


def laplace_logprob_rows(x_hat, target, scale: float):
    """x_hat [R, ...], target [B, ...] with R a multiple of B -> float [R]: row r scored against target row r % B"""
    _dev(x_hat, target)
    rows, tb = x_hat.shape[0], target.shape[0]
    per_row = x_hat.numel() // rows
    assert target.numel() // tb == per_row and rows % tb == 0
    out = torch.empty(rows, dtype=torch.float32, device=x_hat.device)
    _check(lib().mopoe_laplace_logprob_rows(_p(x_hat), _p(target), C.c_int64(rows), C.c_int64(per_row), C.c_int64(tb),
                                            C.c_float(scale), _p(out), _stream()))
    return out


def token_logprob_rows(logp, ids):
    """logp [R, L, V] log-probabilities, ids [B, L] float token ids, R a multiple of B -> float [R]"""
    _dev(logp, ids)
    rows, L, V = logp.shape
    tb = ids.shape[0]
    assert ids.shape[1] == L and rows % tb == 0
    out = torch.empty(rows, dtype=torch.float32, device=logp.device)
    _check(lib().mopoe_token_logprob_rows(_p(logp), _p(ids), C.c_int64(rows), L, V, C.c_int64(tb), _p(out), _stream()))
    return out


def dense_logprob_rows(logp, target):
    """logp [R, L, F] log-probabilities, target [B, L, F] dense / one-hot, R a multiple of B -> float [R]"""
    _dev(logp, target)
    rows, tb = logp.shape[0], target.shape[0]
    per_row = logp[0].numel()
    assert target[0].numel() == per_row and rows % tb == 0
    out = torch.empty(rows, dtype=torch.float32, device=logp.device)
    _check(lib().mopoe_dense_logprob_rows(_p(logp), _p(target), C.c_int64(rows), C.c_int64(per_row), C.c_int64(tb), _p(out), _stream()))
    return out


def lhood_style_sample(mu, logvar, eps, style_mu, style_logvar, style_eps):
    """factorized likelihood estimator, one subset: mu / logvar [B,D], eps [K,B,D]; style_mu / style_logvar [B,S],
    style_eps [K,B,S] -> zcat [K*B, S+D] = [z_style | z] (row k*B + b), t_c [K*B], t_s [K*B] (log N(z;0,I) - log q(z))"""
    _dev(mu, logvar, eps, style_mu, style_logvar, style_eps)
    b, d = mu.shape
    s = style_mu.shape[1]
    k = eps.shape[0]
    if (logvar.shape != mu.shape or tuple(eps.shape) != (k, b, d) or tuple(style_mu.shape) != (b, s)
            or style_logvar.shape != style_mu.shape or tuple(style_eps.shape) != (k, b, s)):
        raise MopoeHipError("lhood_style_sample: mu/logvar [B,D], eps [K,B,D], style_mu/style_logvar [B,S], style_eps [K,B,S]")
    zcat = torch.empty(k * b, s + d, dtype=torch.float32, device=mu.device)
    t_c = torch.empty(k * b, dtype=torch.float32, device=mu.device)
    t_s = torch.empty_like(t_c)
    _check(lib().mopoe_lhood_style_sample(_p(mu), _p(logvar), _p(eps), _p(style_mu), _p(style_logvar), _p(style_eps),
                                          k, b, d, s, _p(zcat), _p(t_c), _p(t_s), _stream()))
    return zcat, t_c, t_s


def lhood_estimates(lp, t_c, t_s, n_samples: int, subset_mask: int):
    """lp: 3-list (PA, Lateral, text) of per-row log p(x_m|z) [K*B]; t_c [K*B]; t_s [K*B] or None; subset_mask: bit m for
    a subset member -> float [4]: the three marginal estimates and the joint"""
    _dev(*lp, t_c, t_s)
    r = t_c.shape[0]
    if r % n_samples or any(t.shape != (r,) for t in (*lp, t_c) + ((t_s,) if t_s is not None else ())):
        raise MopoeHipError("lhood_estimates: every per-row vector must be [K*B]")
    out = torch.empty(4, dtype=torch.float32, device=t_c.device)
    _check(lib().mopoe_lhood_estimates(_ptr3(lp), _p(t_c), _p(t_s), int(n_samples), r // int(n_samples), int(subset_mask),
                                       _p(out), _stream()))
    return out


def logreg_fit(x, y, c: float = 1.0, max_iter: int = 100, tol: float = 1e-5):
    """x [S, N, D] float (one data matrix per subset), y [N, L] float 0/1 -> (W [S, L, D+1] coefficients then intercept,
    info [S, L, 2] = (Newton steps, |grad f|_inf at W)): the optimum of sklearn's LogisticRegression(C=c) problem per
    (subset, label), all S * L fits in one launch.  A problem has converged when info[..., 1] <= tol; the default tol sits
    at what float32 reaches, and a fit that cannot reach it stops where float32 stops improving."""
    _dev(x, y)
    if (x.dim() != 3 or y.dim() != 2 or y.shape[0] != x.shape[1] or x.dtype != torch.float32 or y.dtype != torch.float32
            or y.device != x.device):
        raise MopoeHipError("logreg_fit: x [S,N,D] float32 and y [N,L] float32 on one device")
    s, n, d = x.shape
    l = y.shape[1]
    w = torch.empty(s, l, d + 1, dtype=torch.float32, device=x.device)
    info = torch.empty(s, l, 2, dtype=torch.float32, device=x.device)
    _check(lib().mopoe_logreg_fit(_p(x), _p(y), s, n, d, l, C.c_float(c), int(max_iter), C.c_float(tol), _p(w), _p(info),
                                  _stream()))
    return w, info


def logreg_predict(x, w, want_decision: bool = False):
    """x: [S, M, D] tensor or a sequence of S tensors [M, D]; w [S, L, D+1] -> pred [S, M, L] (1.0 where x . w + b > 0),
    and the decision values [S, M, L] when want_decision"""
    xs = list(x.unbind(0)) if isinstance(x, torch.Tensor) else list(x)
    _dev(w, *xs)
    if (w.dim() != 3 or len(xs) != w.shape[0] or len(xs) > 8 or w.dtype != torch.float32
            or any(t.dim() != 2 or t.shape != xs[0].shape or t.shape[1] + 1 != w.shape[2] or t.dtype != torch.float32
                   or t.device != w.device for t in xs)):
        raise MopoeHipError("logreg_predict: S <= 8 float32 matrices [M,D] and w [S,L,D+1] float32 on one device")
    s, l = w.shape[0], w.shape[1]
    m, d = xs[0].shape
    pred = torch.empty(s, m, l, dtype=torch.float32, device=w.device)
    dec = torch.empty_like(pred) if want_decision else None
    ptrs = (C.c_void_p * s)(*[t.data_ptr() for t in xs])
    _check(lib().mopoe_logreg_predict(ptrs, s, m, d, l, _p(w), _p(pred), _p(dec), _stream()))
    return (pred, dec) if want_decision else pred


def embedding_fwd(ids, table, out_dtype=None):
    _dev(ids, table)
    out_dtype = out_dtype or torch.float32
    out = torch.empty(*ids.shape, table.shape[1], dtype=out_dtype, device=table.device)
    fn = lib().mopoe_embedding_fwd_bf16 if out_dtype == BF16 else lib().mopoe_embedding_fwd
    _check(fn(_p(ids), _p(table), _p(out), C.c_int64(ids.numel()), table.shape[0], table.shape[1], _stream()))
    return out


def embedding_bwd(ids, gout, vocab, padding_idx=0):
    _dev(ids, gout)
    dtable = torch.empty(vocab, gout.shape[-1], dtype=torch.float32, device=gout.device)
    fn = lib().mopoe_embedding_bwd_bf16 if _is16(gout) else lib().mopoe_embedding_bwd
    _check(fn(_p(ids), _p(gout), _p(dtable), C.c_int64(ids.numel()), vocab, gout.shape[-1], padding_idx, _stream()))
    return dtable


# ----------------------------------------------------------------------------------------------
# input pipeline of --weighted_sampler (include/mopoe_hip_data.h, csrc/batch.hip)
# ----------------------------------------------------------------------------------------------
def batch_draw(cdf, seed: int, epoch: int, rank: int, first: int, count: int):
    """cdf: double [n], the inclusive prefix sum of the rows' weights -> int64 [count]: the rows that draws first .. first +
    count - 1 of (seed, epoch, rank) select, with replacement (Philox4x32-10 per draw, binary search in cdf)"""
    _dev(cdf)
    if cdf.dim() != 1 or cdf.numel() < 1 or cdf.dtype != torch.float64:
        raise MopoeHipError("batch_draw: cdf is a float64 vector [n] with n >= 1")
    seed, epoch, rank, first, count = int(seed), int(epoch), int(rank), int(first), int(count)
    if first < 0 or count < 0 or not (0 <= epoch < 1 << 32) or not (0 <= rank < 1 << 32):
        raise MopoeHipError("batch_draw: first >= 0, count >= 0, epoch and rank in [0, 2^32)")
    out = torch.empty(count, dtype=torch.int64, device=cdf.device)
    _check(lib().mopoe_batch_draw(_p(cdf), C.c_int64(cdf.numel()), C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_uint32(epoch),
                                  C.c_uint32(rank), C.c_int64(first), C.c_int64(count), _p(out), _stream()))
    return out


def batch_assemble(pa, lat, text, labels, sel, num_features: Optional[int] = None):
    """pa, lat: uint8 [n,S,S]; text: int32 [n,L] token ids (num_features None) or uint8 [n,L] alphabet positions; labels: float
    [n,n_labels]; sel: int64 [B] row numbers (clamped into [0, n)) -> (PA [B,1,S,S], Lateral [B,1,S,S], text [B,L] or one-hot
    [B,L,num_features], labels [B,n_labels]), all float32: images as u8 / 255 with a correctly rounded division"""
    _dev(pa, lat, text, labels, sel)
    char = num_features is not None
    if (pa.dim() != 3 or pa.shape[1] != pa.shape[2] or lat.shape != pa.shape or pa.dtype != torch.uint8 or lat.dtype != torch.uint8
            or text.dim() != 2 or labels.dim() != 2 or text.shape[0] != pa.shape[0] or labels.shape[0] != pa.shape[0]
            or text.dtype != (torch.uint8 if char else torch.int32) or labels.dtype != torch.float32
            or sel.dim() != 1 or sel.dtype != torch.int64 or sel.numel() < 1 or pa.shape[0] < 1
            or (char and int(num_features) < 1) or any(t.device != pa.device for t in (lat, text, labels, sel))):
        raise MopoeHipError("batch_assemble: pa / lat uint8 [n,S,S], text int32 [n,L] (uint8 with num_features), labels float32 "
                            "[n,n_labels], sel int64 [B] with B >= 1, on one device")
    n, s = pa.shape[0], pa.shape[1]
    l, nl, b = text.shape[1], labels.shape[1], sel.numel()
    f = int(num_features) if char else 0
    out_pa = torch.empty(b, 1, s, s, dtype=torch.float32, device=pa.device)
    out_lat = torch.empty(b, 1, s, s, dtype=torch.float32, device=pa.device)
    out_text = torch.empty(*((b, l, f) if char else (b, l)), dtype=torch.float32, device=pa.device)
    out_labels = torch.empty(b, nl, dtype=torch.float32, device=pa.device)
    _check(lib().mopoe_batch_assemble(_p(pa), _p(lat), C.c_int64(n), s, _p(text), int(char), l, f, _p(labels), nl, _p(sel), b,
                                      _p(out_pa), _p(out_lat), _p(out_text), _p(out_labels), _stream()))
    return out_pa, out_lat, out_text, out_labels


# ----------------------------------------------------------------------------------------------
# profiling hooks used by bench.py
# ----------------------------------------------------------------------------------------------
def prof_enable(on: bool):
    _check(lib().mopoe_prof_enable(int(on)))


def _gather_kinds(t):
    """[(kind, spec)] of the vector-path instantiations of a gather tile (conv_launch.hpp: kind_of_gather)"""
    if t.kernel == "HNONE":
        return []
    specs = (1, 2, 3) if t.bn_form else (1, 3)
    if t.kernel in ("LDS_S", "LDS", "DIRECT"):
        # spec 0 (K no multiple of the chunk) is built where the tuner -- and the decision -- lets such a K reach the tile
        return [(t.kind + spec, spec) for spec in ((0,) if t.k_multiple == 1 else ()) + specs]
    if t.kernel in ("GLDS", "HREG"):
        return [(t.kind + spec - 1, spec) for spec in specs]
    return [(t.kind_bn if spec == 2 else t.kind + (spec == 3), spec) for spec in specs]     # EMU, HGLDS


def _prof_kind_names():
    """kind index -> the kernel's template name as rocprofv3 prints it (header: MOPOE_PROF_KINDS), built from the tile tables;
    None: no kernel has the kind.  The bf16 weight-gradient kinds do not distinguish POW2 and carry the name of the power-of-two
    form (or * for both): see the legend of _WgradTile."""
    names = [None] * 144
    for t in _F32_GATHER_TILES + _BF16_GATHER_TILES:
        for kind, spec in _gather_kinds(t):
            names[kind] = f"{_GATHER_KERNELS[t.kernel]}<{t.targs.format(spec)}>"
        if t.scalar_targs:
            names[32 + t.id] = f"{_GATHER_KERNELS[t.kernel]}<{t.scalar_targs}>"
    for t in _F32_WGRAD_TILES + _BF16_WGRAD_TILES:
        for i, targs in enumerate(t.targs):
            names[t.kind + i] = f"{t.kernel}<{targs}>"
        if t.scalar_targs:
            names[42 + (t.T != 128)] = f"{t.kernel}<{t.scalar_targs}>"
    names[124:130] = ("pw_front_fwd_bf16_kernel<64, false>", "pw_front_fwd_bf16_kernel<64, true>", "pw_front_bwd_bf16_kernel<64>",
                      "pw_front_fwd_f32_kernel<false>", "pw_front_fwd_f32_kernel<true>", "pw_front_bwd_f32_kernel")   # csrc/pointwise.hip
    return names


PROF_KINDS = _prof_kind_names()


def prof_collect():
    """-> {kernel kind: (launches, total ms, total algorithmic flops, total algorithmic bytes)} since the last collect"""
    k = len(PROF_KINDS)
    n, ms, fl, by = (C.c_int64 * k)(), (C.c_double * k)(), (C.c_double * k)(), (C.c_double * k)()
    _check(lib().mopoe_prof_collect(n, ms, fl, by))
    return {name: (n[i], ms[i], fl[i], by[i]) for i, name in enumerate(PROF_KINDS) if name is not None and n[i] > 0}
