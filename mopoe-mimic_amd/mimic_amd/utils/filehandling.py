"""The reference's method switch (mimic/utils/filehandling.py:101-113) under its own name, so that
`from mimic.utils.filehandling import get_method` resolves through the alias package."""
from __future__ import annotations

import argparse

METHODS = ("poe", "moe", "jsd", "joint_elbo")
_FLAG = {"poe": "modality_poe", "moe": "modality_moe", "jsd": "modality_jsd", "joint_elbo": "joint_elbo"}


def get_method(flags: argparse.Namespace) -> argparse.Namespace:
    """Set the boolean that selects flags.method's objective: poe (MVAE; also poe_unimodal_elbos), moe (MMVAE), jsd
    (mixture of experts with a dynamic prior) or joint_elbo (MoPoE).  Unlike the reference, the three method booleans it
    does not select are set to False, so applying it to flags that already name a method switches the method, and an
    unknown name raises (the reference builds the NotImplementedError without raising it)."""
    if flags.method not in _FLAG:
        raise NotImplementedError(f"method {flags.method!r} not implemented: choose one of {', '.join(METHODS)}")
    for name, flag in _FLAG.items():
        setattr(flags, flag, name == flags.method)
    if flags.method == "poe":
        flags.poe_unimodal_elbos = True
    return flags
