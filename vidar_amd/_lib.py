"""ctypes loader for libvidar_hip.so.  There is NO fallback: if the library is missing or a call
fails the product raises, it never routes to a CPU/eager path.

The C ABI is stated once, in `_ABI` below: `declare` turns it into the `argtypes` / `restype` of every entry point, so
call sites pass plain Python ints and floats, tensors' pointers through `ptr`, and a value of the wrong type raises
`ctypes.ArgumentError` instead of being truncated.  A new C entry is declared in include/vidar_hip.h AND in `_ABI`;
tests/test_abi_cpu.py fails until the two agree."""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libvidar_hip.so"
_lib = None
BAD_ARG = -22


class VidarHipError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64.so.7; it must be the copy already loaded when our
        # library is dlopen'ed, otherwise two HIP runtimes fight over the device (hipErrorNoDevice).
        import torch  # noqa: F401
        if not LIB_PATH.exists():
            raise VidarHipError(
                f"{LIB_PATH} not found: build it with `python -m vidar_amd.build` "
                f"(or __graft_entry__.build()); vidar_amd has no CPU fallback")
        _lib = declare(ctypes.CDLL(str(LIB_PATH)))
        dcn = os.environ.get("VIDAR_DCN_VARIANT")                # A/B of the DCNv2 col2im gather (LDS window / global loads)
        if dcn is not None:
            _lib.vidar_dcn_set_variant(int(dcn))
        v3 = os.environ.get("VIDAR_DCNV3_VARIANT")              # A/B of the DCNv3 backward's grad_input accumulation (tools)
        if v3 is not None:
            _lib.vidar_dcnv3_set_variant(int(v3))
        order = os.environ.get("VIDAR_MSDA_ITEM_ORDER")          # A/B of the MSDA gather kernels' item order (tools, bench)
        if order is not None:
            _lib.vidar_msda_set_item_order(int(order))
    return _lib


# Every prototype of include/vidar_hip.h: "<return kind> <parameter kinds in order>", a count in front of a kind repeating it.
#   p = pointer (any pointee, device or host; None = NULL)   i = int   l = int64_t   z = size_t   f = float   u = uint32_t
_KIND = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "z": ctypes.c_size_t, "f": ctypes.c_float,
         "u": ctypes.c_uint32}
_ABI = {
    "vidar_abi_version": "i",
    "vidar_marker": "i i p",
    "vidar_set_deterministic": "i i",
    "vidar_get_deterministic": "i",
    "vidar_dvr_max_d": "i",
    "vidar_dvr_render_forward_f32": "i 6p 8i p",
    "vidar_dvr_render_f32": "i 7p 8i p",
    "vidar_dvr_init_f32": "i 3p 6i p",
    "vidar_dvxlr_max_d": "i",
    "vidar_dvr_set_sort_min_waves": "i i",
    "vidar_dvr_set_traversal": "i i",
    "vidar_dvxlr_set_pad_mode": "i i",
    "vidar_dvxlr_render_f32": "i 8p 7i p",
    "vidar_dvxlr_get_grad_sigma_workspace_bytes": "z 6i",
    "vidar_dvxlr_get_grad_sigma_f32": "i 4p 7i p z p",
    "vidar_dvxlr2_render_f32": "i 11p 7i p",
    "vidar_dvxlr2_get_grad_sigma_f32": "i 7p 7i p z p",
    "vidar_knn1_d3_workspace_bytes": "z 2i",
    "vidar_knn1_d3_fwd": "i 7p 3i p",
    "vidar_knn1_d3_bwd": "i 8p 3i p",
    "vidar_knn1_d3_bwd_workspace_bytes": "i 2i p",
    "vidar_knn1_d3_bwd_ws": "i 8p 3i p z p",
    "vidar_knn_workspace_bytes": "i 6i 2p",
    "vidar_knn_fwd_f32": "i 7p z 6i p",
    "vidar_knn_bwd_f32": "i 8p 5i p",
    "vidar_msda_fwd_f32": "i 6p 7i p",
    "vidar_msda_bwd_workspace_bytes": "z 6i",
    "vidar_msda_set_item_order": "i i",
    "vidar_msda_bwd_f32": "i 9p 7i p z p",
    "vidar_msda_fused_fwd_f32": "i 9p 11i p",
    "vidar_msda_fused_bwd_f32": "i 9p 9i p z p",
    "vidar_drop_add_ln_fwd_f32": "i 8p l i 2f u p",
    "vidar_drop_add_ln_bwd_f32": "i 10p l i f u p",
    "vidar_drop_add_ln_bwd_workspace_bytes": "z l",
    "vidar_relu_drop_fwd_f32": "i 2p l f u p",
    "vidar_relu_drop_bwd_f32": "i 3p l f p",
    "vidar_colsum_f32": "i 2p l i p",
    "vidar_sca_plan_f32": "i 10p 2f 5i p",
    "vidar_sca_rows_f32": "i 5p 6i p",
    "vidar_sca_combine_f32": "i 4p 5i p",
    "vidar_latent_render_bwd_workspace_bytes": "z 5i",
    "vidar_latent_render_prob_fwd_f32": "i 2p 5i f i p",
    "vidar_latent_render_prob_bwd_f32": "i 3p 5i f i p z p",
    "vidar_latent_render_gather_fwd_f32": "i 4p 5i 2f p",
    "vidar_latent_render_gather_bwd_f32": "i 7p 5i 2f p z p",
    "vidar_latent_render_gather_grouped_fwd_f32": "i 4p 6i 2f p",
    "vidar_latent_render_gather_grouped_bwd_f32": "i 7p 6i 2f p z p",
    "vidar_ray_bwd_workspace_bytes": "z 4i",
    "vidar_ray_ce_fwd_f32": "i 7p 6i f p",
    "vidar_ray_ce_bwd_f32": "i 7p 6i f p z p",
    "vidar_ray_gumbel_fwd_f32": "i 7p 6i f p",
    "vidar_ray_gumbel_bwd_f32": "i 7p 6i f p z p",
    "vidar_ray_argmax_f32": "i 6p 6i f p",
    "vidar_ray_dist_fwd_f32": "i 9p 6i f p",
    "vidar_ray_dist_bwd_f32": "i 7p 6i f p z p",
    "vidar_ray_max_k": "i",
    "vidar_ray_force_streamed": "i i",
    "vidar_ray_argmax_cam_f32": "i 3p 4i 4f 4i f p",
    "vidar_cam_rays_f32": "i 3p 4i 4f p",
    "vidar_ray_stats_f32": "i 7p 6i f p",
    "vidar_ray_stats_cam_f32": "i 4p 4i 4f 4i f p",
    "vidar_ray_occupancy_workspace_bytes": "i 4i p",
    "vidar_ray_occupancy_f32": "i 6p 6i f p z p",
    "vidar_ray_occupancy_cam_f32": "i 4p 4i 4f 4i f p z p",
    "vidar_sweep_evidence_f32": "i 5p 6i f p z p",
    "vidar_point_occupancy_f32": "i 5p 6i 2f p",
    "vidar_voxel_occupancy_f32": "i 4p 5i 2f p",
    "vidar_occ_score_workspace_bytes": "i 4i p",
    "vidar_occ_score_f32": "i 4p 4i 3f p z p",
    "vidar_gemm_f32": "i p l i p l i p l 4i 3l 2p i p 2l 3i 2p z p",
    "vidar_gemm_splits": "i 6i",
    "vidar_gemm_workspace_bytes": "z 6i",
    "vidar_gemm_set_variant": "i i",
    "vidar_dcn_set_variant": "i i",
    "vidar_dcn_im2col_f32": "i 4p 11i p",
    "vidar_dcn_col2im_f32": "i 7p 11i p z p",
    "vidar_dcn_col2im_workspace_bytes": "z 7i",
    "vidar_dcn_col2im_det_workspace_bytes": "i 4i p",
    "vidar_conv3x3_few_workspace_bytes": "z i",
    "vidar_conv3x3_few_f32": "i 4p 5i p z p",
    "vidar_affine_act_fwd_f32": "i 5p 4i p",
    "vidar_stem_bn_relu_pool_f32": "i 4p 4i p",
    "vidar_affine_act_bwd_f32": "i 5p 4i p",
    "vidar_dcnv3_set_variant": "i i",
    "vidar_dcnv3_forward_f32": "i 4p 13i f p",
    "vidar_dcnv3_backward_workspace_bytes": "z 13i",
    "vidar_dcnv3_backward_f32": "i 7p 13i f p z p",
    "vidar_det_match_cost_f32": "i 6p 4f 5i p",
    "vidar_det_loss_workspace_bytes": "z 3i",
    "vidar_det_loss_fwd_f32": "i 8p 2f 5i p z p",
    "vidar_det_loss_bwd_f32": "i 10p 2f 5i p",
    "vidar_det_assign_workspace_bytes": "i 4i p",
    "vidar_det_assign_f32": "i 4p 4i p z p",
    "vidar_det_eval_match_f32": "i 10p 7i p",
    "vidar_ray_eval_workspace_bytes": "i i p",
    "vidar_ray_eval_f64": "i 9p 4i p z p",
    "vidar_img_photometric_u8": "i 3p 3i p",
    "vidar_img_photometric_f32": "i 3p 3i p",
    "vidar_img_resample_workspace_bytes": "z 3i",
    "vidar_img_resample_u8": "i 2p 9i p i p 2i p z p",
    "vidar_img_normalise_f32": "i 3p 7i 2p i p",
}


def signature(name):
    """(restype, argtypes) of the entry `name` as `_ABI` states them"""
    ret, *runs = _ABI[name].split()
    return _KIND[ret], [_KIND[r[-1]] for r in runs for _ in range(int(r[:-1] or 1))]


def declare(cdll):
    """Set `argtypes` and `restype` of every entry of `_ABI` on `cdll` (an open libvidar_hip.so); returns `cdll`."""
    for name in _ABI:
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            raise VidarHipError(f"{name} is not exported by {cdll._name}: rebuild the library") from None
        fn.restype, fn.argtypes = signature(name)
    return cdll


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc == BAD_ARG:
        raise ValueError(f"{what}: invalid argument")
    raise VidarHipError(f"{what}: HIP error {rc}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL) as a plain address: the declared pointer parameters take it as it
    is, and no c_void_p object is built per argument (a step makes thousands of these calls).  Only for entries that
    `declare` has typed -- an undeclared ctypes function would cut a bare int to 32 bits."""
    return None if t is None else t.data_ptr()


def workspace(nbytes_fn, *dims, like):
    """Caller-owned device scratch for an op: `nbytes_fn(*dims)` bytes from torch's caching allocator on `like`'s
    device (so it lives on the op's device and stream and is counted by torch's memory statistics).
    -> (tensor or None, pointer, byte count): keep the tensor alive until the call has been enqueued."""
    import torch
    n = nbytes_fn(*dims)
    if n == 0:
        return None, None, 0
    ws = torch.empty(n, dtype=torch.uint8, device=like.device)
    return ws, ptr(ws), n


def stream_of(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


# --------------------------------------------------------------------------------------------------
# optional per-op timing with HIP events on torch's current stream (the stream every op launches on).
# Disabled by default (zero overhead beyond one attribute test); bench.py switches it on to
# measure the dominant kernel live inside the timed region.
# --------------------------------------------------------------------------------------------------
class OpTimer:
    def __init__(self):
        self.enabled = False
        self.records = {}          # name -> list[(start_event, end_event, algorithmic_bytes)]

    def reset(self):
        self.records = {}

    class _Span:
        __slots__ = ("t", "name", "nbytes", "e0")

        def __init__(self, t, name, nbytes):
            self.t, self.name, self.nbytes = t, name, nbytes

        def __enter__(self):
            import torch
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

        def __exit__(self, *exc):
            import torch
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.t.records.setdefault(self.name, []).append((self.e0, e1, self.nbytes))

    class _Null:
        def __enter__(self): return None
        def __exit__(self, *exc): return False

    _null = _Null()

    def span(self, name, nbytes=0):
        return OpTimer._Span(self, name, nbytes) if self.enabled else OpTimer._null

    def summary(self):
        """name -> dict(calls, total_ms, avg_ms, bytes_per_call) ; synchronises."""
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _ in recs]
            out[name] = dict(calls=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms),
                             bytes_per_call=sum(r[2] for r in recs) / len(recs))
        return out


TIMER = OpTimer()
