"""Deterministic mode: order-independent gradient scatters (csrc/det_acc.h).

    from vidar_amd import deterministic
    deterministic.set(True)                      # on; False = off; None = follow torch (the start value)
    with deterministic.use(True): loss.backward()
    deterministic.coverage()                     # what every own op does under the mode

The start value is VIDAR_DETERMINISTIC=0|1; unset (or `set(None)`) the mode follows
torch.are_deterministic_algorithms_enabled() and torch.is_deterministic_algorithms_warn_only_enabled().  The library
switch (vidar_set_deterministic) is process-wide; the ops bring it up to date through `sync()` right before they call
into the library, so flipping torch's flag is enough.

Ops with `not covered` in the table behave as torch's own ops without a deterministic implementation: under the mode
their wrappers raise RuntimeError naming the op (before any GPU call); with warn_only they warn once per op and run the
fp32-atomic form."""
from __future__ import annotations

import contextlib
import os
import warnings

FIXED_POINT = "fixed-point"
FIXED_ORDER = "fixed-order"
ALREADY = "already deterministic"
NOT_COVERED = "not covered"

# op -> (status, entry points / where the order dependence sits)
_COVERAGE = {
    "msda backward": (FIXED_POINT, "vidar_msda_bwd_f32 / vidar_msda_fused_bwd_f32 (grad_value; the plain scatter form)"),
    "ray_ce backward": (FIXED_POINT, "vidar_ray_ce_bwd_f32"),
    "ray_gumbel backward": (FIXED_POINT, "vidar_ray_gumbel_bwd_f32"),
    "ray_dist backward": (FIXED_POINT, "vidar_ray_dist_bwd_f32"),
    "ray_occupancy": (FIXED_POINT, "vidar_ray_occupancy{,_cam}_f32 (hit, free)"),
    "sweep_evidence": (FIXED_POINT, "vidar_sweep_evidence_f32 (hit, free)"),
    "latent_render backward": (FIXED_POINT, "vidar_latent_render_{prob,gather,gather_grouped}_bwd_f32"),
    "knn1_d3 backward": (FIXED_POINT, "vidar_knn1_d3_bwd_ws (grad_p2)"),
    "dcn col2im": (FIXED_POINT, "vidar_dcn_col2im_f32 (grad_x; the plain scatter for every variant)"),
    "drop_add_ln backward": (FIXED_ORDER, "vidar_drop_add_ln_bwd_f32 (dgamma / dbeta: one ordered second stage)"),
    "bias gradient": (FIXED_ORDER, "gemm._colsum / bricks: g2.sum(0) in place of vidar_colsum_f32"),
    "dcnv3 backward": (NOT_COVERED, "vidar_dcnv3_backward_f32 (grad_input)"),
    "dvr.render": (NOT_COVERED, "vidar_dvr_render_f32 (grad_sigma)"),
    "dvxlr.get_grad_sigma": (NOT_COVERED, "vidar_dvxlr_get_grad_sigma_f32"),
    "dvxlr_v2.get_grad_sigma": (NOT_COVERED, "vidar_dvxlr2_get_grad_sigma_f32"),
    "knn generic backward": (NOT_COVERED, "vidar_knn_bwd_f32 (grad_p2); chamferdist._C._generic_knn_backward (scatter_add_) for D > 8 or K > 32"),
    "gemm": (ALREADY, "vidar_gemm_f32: split-K slabs summed in a fixed order"),
    "det_loss": (ALREADY, "vidar_det_loss_{fwd,bwd}_f32"),
    "forward kernels, gathers": (ALREADY, "every forward; grad_sampling_loc / grad_attn_weight; knn grad_p1"),
}

_mode = None          # True / False: set explicitly; None: follow torch
_warn_only = False    # only with an explicit True (use(True, warn_only=True)); torch's own flag otherwise
_warned = set()
_pushed = None        # what sync() last wrote to the library switch (None: nothing yet)


def _from_env():
    v = os.environ.get("VIDAR_DETERMINISTIC")
    if v is None or v == "":
        return None
    if v not in ("0", "1"):
        raise ValueError(f"VIDAR_DETERMINISTIC must be 0 or 1, not {v!r}")
    return v == "1"


_mode = _from_env()


def set(on, warn_only=False):
    """True / False: the mode on / off whatever torch says; None: follow torch's flags.  -> the previous setting"""
    global _mode, _warn_only
    if on is not None and not isinstance(on, (bool, int)):
        raise TypeError("deterministic.set takes True, False or None")
    was = _mode
    _mode = None if on is None else bool(on)
    _warn_only = bool(warn_only) and _mode is True
    _push()
    return was


def _push():
    """an already loaded library learns of an explicit change at once (direct callers of the C ABI do not `sync`)"""
    global _pushed
    from . import _lib
    if _lib._lib is not None:
        _pushed = None                # write it whatever sync() believes the library holds
        sync()


def enabled():
    """Is the mode on for the next op?"""
    if _mode is not None:
        return _mode
    import torch
    return torch.are_deterministic_algorithms_enabled()


def warn_only():
    if _mode is not None:
        return _warn_only
    import torch
    return torch.is_deterministic_algorithms_warn_only_enabled()


@contextlib.contextmanager
def use(on, warn_only=False):
    """The mode `on` (True / False / None) inside the block; the previous setting comes back after it."""
    global _mode, _warn_only
    saved = (_mode, _warn_only)
    set(on, warn_only)
    try:
        yield
    finally:
        _mode, _warn_only = saved
        _push()


def sync():
    """Bring the library's process-wide switch up to date; the covered ops call this before they ask the library for
    their workspace.  -> is the mode on"""
    global _pushed
    on = enabled()
    if on != _pushed:                 # one comparison per op in the steady state, no call into the library
        from ._lib import lib
        lib().vidar_set_deterministic(int(on))
        _pushed = on
    return on


def require(op):
    """Called by the wrapper of an op that has no deterministic form, before it touches the GPU."""
    if not enabled():
        return
    status = _COVERAGE[op][0]
    assert status == NOT_COVERED, op
    msg = (f"vidar_amd: {op} ({_COVERAGE[op][1]}) does not have a deterministic implementation, but the deterministic "
           f"mode is on (vidar_amd.deterministic / torch.use_deterministic_algorithms)")
    if not warn_only():
        raise RuntimeError(msg + "; turn the mode off for this op or pass warn_only=True")
    if op not in _warned:
        _warned.add(op)
        warnings.warn(msg + "; running its fp32-atomic form", UserWarning, stacklevel=3)


def warned():
    """The uncovered ops that have warned so far (tools/determinism_report.py)."""
    return sorted(_warned)


def coverage():
    """[(op, status, entry points)] for every own op; status is one of
    'fixed-point', 'fixed-order', 'already deterministic', 'not covered'."""
    return [(op, status, where) for op, (status, where) in _COVERAGE.items()]


def coverage_table():
    """coverage() as the markdown table of the README"""
    rows = ["| op | under the mode | entry points |", "|---|---|---|"]
    rows += [f"| {op} | {status} | `{where}` |" for op, status, where in coverage()]
    return "\n".join(rows)
