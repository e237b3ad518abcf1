"""Per-kernel timing of the HIP ops at BASELINE sizes (HIP events on torch's current stream, which
is the stream every op launches on).  Prints one JSON line per op: ms, algorithmic GB/s."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timeit(fn, warm=3, it=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


def report(name, ms, nbytes=None, **kw):
    d = {"op": name, "ms": round(ms, 4)}
    if nbytes:
        d["alg_MB"] = round(nbytes / 1e6, 2); d["GBps"] = round(nbytes / ms / 1e6, 1)
        d["frac_8TBps"] = round(nbytes / ms / 1e6 / 8000, 4)
    d.update(kw)
    print(json.dumps(d), flush=True)


PAD_MODE_DEFAULT = 1


def bench_dvr(which):
    buf = torch.empty(2478800000 // 4, device="cuda")
    ms = timeit(lambda: buf.zero_())
    report("device fill 2.48 GB (write ceiling)", ms, buf.numel() * 4)
    src = torch.empty_like(buf)
    ms = timeit(lambda: buf.copy_(src))
    report("device copy 2.48 GB (read+write bytes)", ms, buf.numel() * 8)
    del buf, src
    from vidar_amd.synthetic import ray_set
    from vidar_amd.third_lib import dvr, dvxlr, dvxlr_v2
    from vidar_amd._lib import lib
    t = lambda a: torch.from_numpy(a).cuda()
    # A/B of the launch variants (results are identical, tests/test_dvr_gpu.py)
    sigma, origin, points, tindex = map(t, ray_set(seed=0, N=1, T=5, rays_per_frame=30000))
    for pad_mode in (0, 1):
        for thr, order in ((1 << 30, "plain"), (0, "ranked")):
            lib().vidar_dvxlr_set_pad_mode(pad_mode); lib().vidar_dvr_set_sort_min_waves(thr)
            ms = timeit(lambda: dvxlr.render(sigma, origin, points, tindex))
            ms2 = timeit(lambda: dvxlr_v2.render_v2(sigma, origin, points, tindex, sigma))
            ms3 = timeit(lambda: dvr.render_forward(sigma, origin, points, tindex, [5, 16, 200, 200], "train"))
            report(f"A/B pad_mode={pad_mode} order={order} M=150000", ms, render_v2_ms=round(ms2, 4),
                   render_forward_ms=round(ms3, 4))
    sigma, origin, points, tindex = map(t, ray_set(seed=0, N=1, T=1, rays_per_frame=30000))
    for pad_mode in (0, 1):
        lib().vidar_dvxlr_set_pad_mode(pad_mode); lib().vidar_dvr_set_sort_min_waves(1024)
        ms = timeit(lambda: dvxlr.render(sigma, origin, points, tindex), it=30)
        ms2 = timeit(lambda: dvxlr_v2.render_v2(sigma, origin, points, tindex, sigma), it=30)
        report(f"A/B pad_mode={pad_mode} M=30000", ms, render_v2_ms=round(ms2, 4))
    lib().vidar_dvxlr_set_pad_mode(PAD_MODE_DEFAULT); lib().vidar_dvr_set_sort_min_waves(1024)
    for T, rpf in ((1, 30000), (5, 30000)):
        sigma, origin, points, tindex = map(t, ray_set(seed=0, N=1, T=T, rays_per_frame=rpf))
        N, M = tindex.shape
        vol = sigma.numel() * 4
        out = dvxlr.render(sigma, origin, points, tindex)
        cnt = int(((out[3] != 0).any(-1)).sum())
        ms = timeit(lambda: dvxlr.render(sigma, origin, points, tindex))
        report(f"dvxlr.render T={T} M={M}", ms, vol + N * M * 16 + N * M * 4 * (2 + 1026 * 4), samples=cnt)
        em = out[2] * 0.5
        ms = timeit(lambda: dvxlr.get_grad_sigma(em, out[3], tindex, sigma))
        report(f"dvxlr.get_grad_sigma T={T} M={M}", ms, N * M * 1026 * 16 + 2 * vol)
        ms = timeit(lambda: dvr.render_forward(sigma, origin, points, tindex, [T, 16, 200, 200], "train"))
        report(f"dvr.render_forward T={T} M={M}", ms, vol + N * M * 24 + cnt * 4)
        ms = timeit(lambda: dvr.render(sigma, origin, points, tindex, "l1"))
        report(f"dvr.render T={T} M={M}", ms, 2 * vol + N * M * 24 + cnt * 12)
        ms = timeit(lambda: dvxlr_v2.render_v2(sigma, origin, points, tindex, sigma))
        report(f"dvxlr_v2.render_v2 T={T} M={M}", ms, 2 * vol + N * M * 16 + N * M * 4 * (2 + 1026 * 6))
        del out, em


def bench_dvr_trav(which):
    """lane-per-ray kernels (traversal 0) vs the step-parallel kernels (traversal 1, csrc/dvr_par.h) per op and ray
    count; results are identical (tests/test_dvr_gpu.py)."""
    from vidar_amd.synthetic import ray_set
    from vidar_amd.third_lib import dvr, dvxlr, dvxlr_v2
    from vidar_amd._lib import lib
    t = lambda a: torch.from_numpy(a).cuda()
    for T, rpf in ((1, 30000), (2, 30000), (3, 30000), (5, 30000)):
        sigma, origin, points, tindex = map(t, ray_set(seed=0, N=1, T=T, rays_per_frame=rpf))
        N, M = tindex.shape
        vol = sigma.numel() * 4
        lib().vidar_dvr_set_traversal(0)
        cnt = int(((dvxlr.render(sigma, origin, points, tindex)[3] != 0).any(-1)).sum())
        ops = {
            "dvr.render_forward": (lambda: dvr.render_forward(sigma, origin, points, tindex, [T, 16, 200, 200], "train"),
                                   vol + N * M * 24 + cnt * 4),
            "dvr.render": (lambda: dvr.render(sigma, origin, points, tindex, "l1"), 2 * vol + N * M * 24 + cnt * 12),
            "dvxlr.render": (lambda: dvxlr.render(sigma, origin, points, tindex),
                             vol + N * M * 16 + N * M * 4 * (2 + 1026 * 4)),
            "dvxlr_v2.render_v2": (lambda: dvxlr_v2.render_v2(sigma, origin, points, tindex, sigma),
                                   2 * vol + N * M * 16 + N * M * 4 * (2 + 1026 * 6)),
        }
        for name, (fn, nbytes) in ops.items():
            ms = {}
            for trav in (0, 1):
                lib().vidar_dvr_set_traversal(trav)
                ms[trav] = timeit(fn, it=30)
            report(f"{name} M={M}", ms[1], nbytes, lane_per_ray_ms=round(ms[0], 4), step_parallel_ms=round(ms[1], 4),
                   samples=cnt)
    lib().vidar_dvr_set_traversal(-1)


def bench_knn(which):
    from vidar_amd.third_lib.chamferdist import knn_points
    rng = np.random.default_rng(0)
    for P1, P2 in ((30000, 30000), (10000, 30000), (30000, 10000)):
        a = torch.from_numpy(rng.uniform(-50, 50, (1, P1, 3)).astype(np.float32)).cuda()
        b = torch.from_numpy(rng.uniform(-50, 50, (1, P2, 3)).astype(np.float32)).cuda()
        ms = timeit(lambda: knn_points(a, b))
        report(f"knn1_d3 {P1}x{P2}", ms, 12 * (P1 + P2) + 12 * P1, Gpairs_s=round(P1 * P2 / ms / 1e6, 1),
               fp32_TFLOPs=round(P1 * P2 * 8 / ms / 1e9, 2))
    bench_knn_generic(rng)


def bench_knn_generic(rng):
    """every other (D, K): the kernels of csrc/knn_generic.hip next to the torch program they replace (the parent's
    path, VIDAR_KNN_GENERIC=torch), alternating in one run: time, Gpairs/s and peak temporary bytes of both (torch's
    allocator statistics: the peak above what was allocated before the call, less the two outputs)"""
    from vidar_amd.third_lib.chamferdist import _C

    def peak_temp(fn, out_bytes):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before - out_bytes

    for P1, P2 in ((30000, 30000), (10000, 30000)):
        for D, K in ((3, 2), (3, 4), (3, 8), (3, 32), (8, 4), (2, 1)):
            a = torch.from_numpy(rng.uniform(-50, 50, (1, P1, D)).astype(np.float32)).cuda()
            b = torch.from_numpy(rng.uniform(-50, 50, (1, P2, D)).astype(np.float32)).cuda()
            l1 = torch.tensor([P1], device="cuda"); l2 = torch.tensor([P2], device="cuda")
            fwd = lambda: _C.knn_points_idx(a, b, l1, l2, K, -1)
            idx, dist = fwd()
            gd = torch.from_numpy(rng.standard_normal((1, P1, K)).astype(np.float32)).cuda()
            cases = [("fwd", fwd, 12 * P1 * K, P1 * P2)]
            if K == 8:
                cases.append(("bwd", lambda: _C.knn_points_backward(a, b, l1, l2, idx, gd), 4 * D * (P1 + P2), P1 * K))
            for what, fn, out_bytes, pairs in cases:
                res = {}
                for path in ("kernel", "torch", "kernel", "torch"):           # alternating; the better of two windows each
                    if path == "torch":
                        os.environ["VIDAR_KNN_GENERIC"] = "torch"
                    try:
                        ms = timeit(fn, warm=1, it=3) if path == "torch" else timeit(fn)
                        res[path] = (min(ms, res[path][0]) if path in res else ms, peak_temp(fn, out_bytes))
                    finally:
                        os.environ.pop("VIDAR_KNN_GENERIC", None)
                if what == "fwd":                                             # the two paths give the same bytes
                    os.environ["VIDAR_KNN_GENERIC"] = "torch"
                    try:
                        ti, td = fn()
                    finally:
                        os.environ.pop("VIDAR_KNN_GENERIC", None)
                    assert torch.equal(ti, idx) and torch.equal(td, dist), (D, K, P1, P2)
                (kms, ktemp), (tms, ttemp) = res["kernel"], res["torch"]
                report(f"knn_generic {what} D={D} K={K} {P1}x{P2}", kms, None, torch_ms=round(tms, 3),
                       speedup=round(tms / kms, 1), Gpairs_s=round(pairs / kms / 1e6, 2),
                       torch_Gpairs_s=round(pairs / tms / 1e6, 2), temp_MB=round(ktemp / 1e6, 2),
                       torch_temp_MB=round(ttemp / 1e6, 2))


def bench_msda_coherent(which):
    """both scatter strategies of msda_bwd on spatially coherent queries (what the model produces:
    neighbouring BEV queries sample next to each other; the random reference points of `bench_msda`
    share no lines) + their agreement."""
    from vidar_amd.synthetic import msda_operands_coherent
    from vidar_amd.plugin.modules.multi_scale_deformable_attn_function import _msda_backward, _msda_forward
    fpn = [(116, 200), (58, 100), (29, 50), (15, 25)]
    for name, B, shapes, Nq, P, px in (("TSA-like", 2, [(200, 200)], 40000, 4, 1.0),
                                       ("SCA-like far (2 level-0 px between queries)", 6, fpn, 10000, 8, 2.0),
                                       ("SCA-like near (8 px)", 6, fpn, 10000, 8, 8.0)):
        value, sh, lsi, loc, w = msda_operands_coherent(0, B, shapes, Nq, P=P, px=px, device="cuda")
        report(f"msda_fwd {name}", timeit(lambda: _msda_forward(value, sh, lsi, loc, w)))
        go = torch.randn(B, Nq, 256, device="cuda")
        outs = {}
        for binned in (False, True):
            outs[binned] = _msda_backward(value, sh, lsi, loc, w, go, binned=binned)
            ms = timeit(lambda: _msda_backward(value, sh, lsi, loc, w, go, binned=binned))
            report(f"msda_bwd {name} binned={binned}", ms)
        for a, b, nm in zip(outs[False], outs[True], ("grad_value", "grad_loc", "grad_w")):
            print(json.dumps({"agreement": nm, "max_abs_diff": float((a - b).abs().max()),
                              "scale": float(a.abs().max())}), flush=True)


def bench_msda(which):
    from vidar_amd.synthetic import msda_operands
    from vidar_amd.plugin.modules.multi_scale_deformable_attn_function import _msda_forward, _msda_backward
    fpn = [(116, 200), (58, 100), (29, 50), (15, 25)]
    for name, B, shapes, Nq, P in (("TSA", 2, [(200, 200)], 40000, 4), ("SCA", 6, fpn, 10000, 8),
                                   ("Pred", 1, [(200, 200)], 40000, 4)):
        value, sh, lsi, loc, w = msda_operands(0, B, shapes, Nq, P=P, device="cuda")
        L = len(shapes); Nv = value.shape[1]
        fwd_bytes = 4 * (B * Nv * 256 + B * Nq * 8 * L * P * 3 + B * Nq * 256)
        ms = timeit(lambda: _msda_forward(value, sh, lsi, loc, w))
        report(f"msda_fwd {name}", ms, fwd_bytes)
        go = torch.randn(B, Nq, 256, device="cuda")
        for binned in (False, True):
            ms = timeit(lambda: _msda_backward(value, sh, lsi, loc, w, go, binned=binned))
            report(f"msda_bwd {name} binned={binned}", ms, fwd_bytes + 4 * (B * Nq * 256 + B * Nv * 256 + B * Nq * 8 * L * P * 3))


def bench_msda_sca(which):
    """SpatialCrossAttention shape only, few iterations: the driver of the PMC passes (tools/pmc_pass.sh)"""
    from vidar_amd.synthetic import msda_operands
    from vidar_amd.plugin.modules.multi_scale_deformable_attn_function import _msda_forward, _msda_backward
    fpn = [(116, 200), (58, 100), (29, 50), (15, 25)]
    value, sh, lsi, loc, w = msda_operands(0, 6, fpn, 10000, P=8, device="cuda")
    go = torch.randn(6, 10000, 256, device="cuda")
    report("msda_fwd SCA", timeit(lambda: _msda_forward(value, sh, lsi, loc, w), warm=1, it=3))
    report("msda_bwd SCA binned=True", timeit(lambda: _msda_backward(value, sh, lsi, loc, w, go, binned=True), warm=1, it=3))


def bench_msda_sca_coherent(which):
    """SpatialCrossAttention shape on spatially COHERENT queries (neighbouring queries sample 8 level-0 pixels apart: what
    the model's projected BEV pillars look like), few iterations: the driver of the PMC passes whose traffic is paired
    with the in-model kernel time in bench.py's `roofline.traffic`"""
    from vidar_amd.synthetic import msda_operands_coherent
    from vidar_amd.plugin.modules.multi_scale_deformable_attn_function import _msda_backward, _msda_forward
    fpn = [(116, 200), (58, 100), (29, 50), (15, 25)]
    import os
    nq = int(os.environ.get("VIDAR_KBENCH_NQ", "10000"))      # 7680 = the padded visible-query count of the bench's step
    value, sh, lsi, loc, w = msda_operands_coherent(0, 6, fpn, nq, P=8, px=8.0, device="cuda")
    go = torch.randn(6, nq, 256, device="cuda")
    report("msda_fwd SCA coherent", timeit(lambda: _msda_forward(value, sh, lsi, loc, w), warm=1, it=3))
    report("msda_bwd SCA coherent binned=True", timeit(lambda: _msda_backward(value, sh, lsi, loc, w, go, binned=True), warm=1, it=3))


def bench_dcn(which):
    """DCNv2 sampling kernels at the backbone shapes (stage 3: 256 ch 58x100 with the 6 gradient images / the 24 history
    images, stage 4: 512 ch 29x50), offsets at init (0) and trained-like (N(0, (1.5 px)^2), vidar_amd/weights.py);
    $VIDAR_KBENCH_DCN_STD overrides the list."""
    import os
    from vidar_amd.plugin.backbones import dcn_col2im
    from vidar_amd._lib import lib, check, ptr, stream_of
    g = torch.Generator().manual_seed(0)
    stds = [float(v) for v in os.environ.get("VIDAR_KBENCH_DCN_STD", "0,1.5,-1.5").split(",")]     # negative: SMOOTH offsets
    for N, C, H, W in ((6, 256, 58, 100), (24, 256, 58, 100), (6, 512, 29, 50)):
        x = torch.randn(N, C, H, W, generator=g).cuda()
        mask = torch.rand(N, 9, H, W, generator=g).cuda()
        gcols = torch.randn(N, C * 9, H * W, generator=g).cuda()
        cols = torch.empty_like(gcols)
        for std in stds:
            off = torch.randn(N, 18, H, W, generator=g)
            if std < 0:       # spatially smooth like a convolution's output (the model's conv_offset): 7x7 box-filtered noise
                off = torch.nn.functional.avg_pool2d(off, 7, stride=1, padding=3)
                off = off / off.std()
            off = (off * abs(std)).cuda()
            tag = f"N={N} C={C} {H}x{W} offsets~{abs(std)}px" + (" smooth" if std < 0 else "")
            ms = timeit(lambda: check(lib().vidar_dcn_im2col_f32(ptr(x), ptr(off), ptr(mask), ptr(cols), N, C, H, W, H, W,
                                                                 3, 3, 1, 1, 1, stream_of(x)), "im2col"))
            report(f"dcn_im2col {tag}", ms, 4 * (x.numel() + cols.numel() + off.numel() + mask.numel()))
            if N > 6:
                continue                      # the history images carry no gradients
            for gather in (False, True):
                ms = timeit(lambda: dcn_col2im(gcols, x, off, mask, 3, 3, 1, 1, 1, H, W, gather=gather))
                report(f"dcn_col2im {tag} gather={gather}", ms,
                       4 * (3 * x.numel() + gcols.numel() + 2 * off.numel() + 2 * mask.numel()))


def bench_dcnv3(which):
    """DCNv3 forward / backward (csrc/dcnv3.hip) at the four stage shapes of InternImage-T and -B for 6 cameras at
    928 x 1600 (3x3, stride 1, pad 1; gc = 16), trained-like offsets N(0, (1.5 px)^2) and softmax masks, next to the same
    call through `dcnv3_core_pytorch` (torch's grid_sample, what `DCNv3_pytorch` runs) as the comparison line.  The two are
    ALTERNATED in the same process: 5 rounds of (HIP x n, torch x m) after a warm-up of both, n / m sized so that a group spans >= 5 ms; the line reports the
    median round and the spread (min .. max) of the rounds.  The torch backward is autograd's backward alone (the graph is
    built outside the timed region)."""
    from vidar_amd.plugin.ops_dcnv3 import dcnv3_core_pytorch
    from vidar_amd.third_lib import dcnv3
    from vidar_amd._lib import lib
    g = torch.Generator().manual_seed(0)
    prev = lib().vidar_dcnv3_set_variant(-1)
    print(json.dumps({"dcnv3_backward_variant": prev}), flush=True)
    rounds = 5
    N, P = 6, 9

    def alternate(fa, fb):
        # every timed group spans at least ~5 ms of device time (5 .. 100 launches, from the warm-up's own timing)
        reps = lambda ms: int(min(100, max(5, 5.0 / max(ms, 1e-3))))
        ia, ib = reps(timeit(fa, warm=2, it=3)), reps(timeit(fb, warm=2, it=3))
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timeit(fa, warm=0, it=ia)); tb.append(timeit(fb, warm=0, it=ib))
        return sorted(ta), sorted(tb)

    for model, c0, g0 in (("T", 64, 4), ("B", 112, 7)):
        for i, (H, W) in enumerate(((232, 400), (116, 200), (58, 100), (29, 50))):
            C, G = c0 << i, g0 << i
            gc = C // G
            geo = (3, 3, 1, 1, 1, 1, 1, 1, G, gc, 1.0)
            x = torch.randn(N, H, W, C, generator=g).cuda()
            off = (torch.randn(N, H, W, G * P * 2, generator=g) * 1.5).cuda()
            mask = torch.softmax(torch.randn(N, H, W, G, P, generator=g), -1).reshape(N, H, W, G * P).cuda()
            gout = torch.randn(N, H, W, C, generator=g).cuda()
            tag = f"InternImage-{model} stage {i} N={N} {H}x{W} C={C} G={G}"
            fwd_bytes = 4 * (2 * x.numel() + off.numel() + mask.numel())
            bwd_bytes = 4 * (4 * x.numel() + 2 * off.numel() + 2 * mask.numel())    # reads x, grad_out; zeroes + writes grad_input

            def torch_fwd():
                with torch.no_grad():
                    return dcnv3_core_pytorch(x, off, mask, *geo)
            th, tt = alternate(lambda: dcnv3.dcnv3_forward(x, off, mask, *geo, 256), torch_fwd)
            mid = rounds // 2
            report(f"dcnv3_fwd {tag}", th[mid], fwd_bytes, min_ms=round(th[0], 4), max_ms=round(th[-1], 4))
            report(f"dcnv3_fwd grid_sample {tag}", tt[mid], fwd_bytes, min_ms=round(tt[0], 4), max_ms=round(tt[-1], 4),
                   ratio_vs_hip=round(tt[mid] / th[mid], 2), faster_beyond_spread=bool(th[-1] < tt[0]))
            ops = [t.clone().requires_grad_(True) for t in (x, off, mask)]
            y = dcnv3_core_pytorch(*ops, *geo)
            th, tt = alternate(lambda: dcnv3.dcnv3_backward(x, off, mask, *geo, gout, 256),
                               lambda: torch.autograd.grad(y, ops, gout, retain_graph=True))
            report(f"dcnv3_bwd {tag}", th[mid], bwd_bytes, min_ms=round(th[0], 4), max_ms=round(th[-1], 4))
            report(f"dcnv3_bwd grid_sample {tag}", tt[mid], bwd_bytes, min_ms=round(tt[0], 4), max_ms=round(tt[-1], 4),
                   ratio_vs_hip=round(tt[mid] / th[mid], 2), faster_beyond_spread=bool(th[-1] < tt[0]))
            del y, ops
            torch.cuda.empty_cache()


def bench_affine(which):
    """Frozen BN + (residual) + ReLU of the backbone (csrc/affine_act.hip) at the stage-3 shapes of the 24 history images."""
    from vidar_amd.plugin.backbones import FrozenBN
    for C, res in ((1024, True), (256, False)):
        bn = FrozenBN(C).cuda()
        x = torch.randn(24, C, 58, 100, device="cuda")
        r = torch.randn_like(x) if res else None
        with torch.no_grad():
            ms = timeit(lambda: bn(x, residual=r, relu=True))
        report(f"affine_act_fwd [24,{C},58,100] residual={res}", ms, 4 * x.numel() * (3 if res else 2))


def bench_stem(which):
    """The ResNet stem at the 24 history images: conv1 (MIOpen's 7x7 / stride 2), and BN + ReLU + max-pool as affine_act +
    torch's pooling vs the one-pass kernel the backbone uses."""
    import torch.nn as nn
    import torch.nn.functional as F
    from vidar_amd.plugin.backbones import FrozenBN, stem_bn_relu_pool
    conv = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda()
    conv.weight.requires_grad = False
    bn = FrozenBN(64).cuda()
    x = torch.randn(24, 3, 928, 1600, device="cuda")
    flops = 2 * 24 * 64 * 464 * 800 * 147
    with torch.no_grad():
        ms = timeit(lambda: conv(x))
        print(json.dumps({"op": "stem conv1 7x7 stride 2 (MIOpen)", "ms": round(ms, 4), "TFLOPs": round(flops / ms / 1e9, 1)}))
        y = conv(x)
        nb = 4 * (y.numel() + y.numel() // 4)
        report("stem bn+relu+pool two kernels", timeit(lambda: F.max_pool2d(bn(y, relu=True), 3, stride=2, padding=1)), nb)
        report("stem bn+relu+pool one pass", timeit(lambda: stem_bn_relu_pool(y, bn)), nb)


def bench_norm(which):
    """LayerNorm(dropout(x) + residual) on a [40000, 256] BEV map: fused HIP kernels vs torch's three ops."""
    import torch.nn as nn
    import torch.nn.functional as F
    from vidar_amd.plugin.bricks import drop_add_layernorm
    norm = nn.LayerNorm(256).cuda()
    x = torch.randn(1, 40000, 256, device="cuda", requires_grad=True)
    r = torch.randn(1, 40000, 256, device="cuda", requires_grad=True)
    gy = torch.randn(1, 40000, 256, device="cuda")
    nb = x.numel() * 4
    for name, fn in (("fused", lambda: drop_add_layernorm(x, r, norm, 0.1, True)),
                     ("torch", lambda: norm(F.dropout(x, 0.1, True) + r))):
        ms = timeit(lambda: fn())
        report(f"drop_add_ln fwd {name}", ms, 3 * nb)
        y = fn()
        ms = timeit(lambda: torch.autograd.grad(y, [x, r, norm.weight, norm.bias], gy, retain_graph=True))
        report(f"drop_add_ln bwd {name}", ms, 4 * nb)


def _lr_geometry(H, W, G, step, dev):
    """waypoints of every cell's ray in [-1, 1] (the cell itself last), their lengths and the border bound"""
    ys, xs = torch.meshgrid((torch.arange(H, device=dev) + 0.5) / H, (torch.arange(W, device=dev) + 0.5) / W, indexing="ij")
    grids = torch.stack((xs.reshape(-1), ys.reshape(-1)), -1)[None]
    r = grids - 0.5
    rn = torch.nan_to_num(r / r.norm(dim=-1, keepdim=True))
    steps = (torch.arange(G, device=dev) + 0.5) * (step / (min(H, W) // 2))
    path = torch.cat([0.5 + rn[:, :, None] * steps.view(1, 1, -1, 1), grids[:, :, None]], 2) * 2 - 1
    bound = torch.minimum(1 / rn[..., 0:1].abs(), 1 / rn[..., 1:2].abs())
    return path, path.norm(dim=-1, keepdim=True), bound


def _lr_torch(occ, a, G, step):
    """the op chain the two kernels replace, through F.grid_sample on the GPU: occ [1,H,W,Z], a [1,H,W,A] -> prob, feat"""
    import torch.nn.functional as F
    bs, H, W, Z = occ.shape
    A = a.shape[-1]
    path, length, bound = _lr_geometry(H, W, G, step, occ.device)
    p = torch.sigmoid(F.grid_sample(occ.permute(0, 3, 1, 2), path, align_corners=False).permute(0, 2, 3, 1))
    trans = torch.cumprod(1 - p * (length < length[..., -1:, :]), dim=2)
    prob = (trans[..., -1, :] * p[..., -1, :]).view(bs, H, W, Z)
    path = path[..., :-1, :].contiguous()
    av = F.grid_sample(a.permute(0, 3, 1, 2), path, align_corners=False).view(bs, Z, A // Z, H * W, G)
    m = F.grid_sample(prob.permute(0, 3, 1, 2), path, align_corners=False) * (length[..., :-1, 0] < bound).view(bs, 1, H * W, G)
    m = (m / (m.sum(-1, keepdim=True) + 1e-3)).view(bs, Z, 1, H * W, G)
    return prob, (av * m).sum(-1).view(bs, A, H * W).permute(0, 2, 1).reshape(bs, H, W, A)


def bench_lr(which):
    """the four LatentRendering kernels at 200 x 200, 256 waypoints: the released 16 bins / 16 LoRA channels first (the
    rows every earlier log has), then other (Z, A) with the same chain through F.grid_sample next to them.  Algorithmic
    bytes: every map read or written once (Z floats per cell for occ / prob / msum and their gradients, A for a / feat)."""
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import _PathProb, _RayGather
    Q = 40000

    def rows(Z, A, step, tag="", it=10):
        occ = torch.randn(1, 200, 200, Z, device="cuda", requires_grad=True)
        a = torch.randn(1, 200, 200, A, device="cuda", requires_grad=True)
        ms = timeit(lambda: _PathProb.apply(occ, 256, step, 0), it=it)
        report(f"lr_prob_fwd{tag} step={step}", ms, 4 * Q * 2 * Z)
        p = _PathProb.apply(occ, 256, step, 0)
        g = torch.randn_like(p)
        ms = timeit(lambda: torch.autograd.grad(p, occ, g, retain_graph=True), it=it)
        report(f"lr_prob_bwd{tag} step={step}", ms, 4 * Q * 3 * Z)
        pd = p.detach().requires_grad_(True)
        ms = timeit(lambda: _RayGather.apply(pd, a, 256, step, 1e-3), it=it)
        report(f"lr_gather_fwd{tag} step={step}", ms, 4 * Q * (2 * Z + 2 * A))
        f = _RayGather.apply(pd, a, 256, step, 1e-3)
        ga = torch.randn_like(f)
        ms = timeit(lambda: torch.autograd.grad(f, [pd, a], ga, retain_graph=True), it=it)
        report(f"lr_gather_bwd{tag} step={step}", ms, 4 * Q * (3 * Z + 4 * A))
        return occ, a, g, ga

    for step in (1.0, 0.5):
        rows(16, 16, step)
    for Z, A in ((1, 16), (4, 16), (32, 32), (16, 64)):
        for step in (1.0, 0.5):
            occ, a, g, ga = rows(Z, A, step, f" Z={Z} A={A}", it=20)
            fwd_bytes, bwd_bytes = 4 * Q * (4 * Z + 2 * A), 4 * Q * (6 * Z + 4 * A)
            ms = timeit(lambda: _lr_torch(occ.detach(), a.detach(), 256, step), warm=1, it=3)
            report(f"lr fwd (both stages) grid_sample Z={Z} A={A} step={step}", ms, fwd_bytes)
            prob, feat = _lr_torch(occ, a, 256, step)
            ms = timeit(lambda: torch.autograd.grad([prob, feat], [occ, a], [g, ga], retain_graph=True), warm=1, it=3)
            report(f"lr bwd (both stages) grid_sample Z={Z} A={A} step={step}", ms, bwd_bytes)
            del prob, feat
            torch.cuda.empty_cache()


def bench_ray(which):
    from vidar_amd.plugin.dense_heads.ray_ops import ray_ce, ray_gumbel, gumbel_noise
    from vidar_amd.synthetic import ray_set
    sig, origin, points, tindex = ray_set(seed=0, N=1, T=1, rays_per_frame=30000)
    sigma = torch.randn(1, 16, 200, 200, device="cuda", requires_grad=True)
    o, p, ti = (torch.from_numpy(a[0]).cuda() for a in (origin, points, tindex))
    ms = timeit(lambda: ray_ce(sigma, o, p, ti))
    report("ray_ce_fwd P=30000", ms, 4 * (16 * 200 * 200 + 30000 * 5), Mrays_s=round(30000 / ms / 1e3, 1))
    ce, valid = ray_ce(sigma, o, p, ti)
    g = torch.ones_like(ce)
    ms = timeit(lambda: torch.autograd.grad(ce, sigma, g, retain_graph=True))
    report("ray_ce_bwd P=30000", ms, 4 * (2 * 16 * 200 * 200 + 30000 * 5))
    from vidar_amd.synthetic import dense_rays
    pts, tix = dense_rays(1, 16, 200, 200, "cuda")
    noise = gumbel_noise(pts.shape[0], 512)
    ms = timeit(lambda: ray_gumbel(sigma, o, pts, tix, noise))
    report(f"ray_gumbel_fwd R={pts.shape[0]}", ms, 4 * (16 * 200 * 200 + pts.shape[0] * 516))
    d = ray_gumbel(sigma, o, pts, tix, noise)
    ms = timeit(lambda: torch.autograd.grad(d, sigma, torch.ones_like(d), retain_graph=True))
    report(f"ray_gumbel_bwd R={pts.shape[0]}", ms, 4 * (2 * 16 * 200 * 200 + pts.shape[0] * 4))
    # any ray_grid_num (the streamed kernels) next to the register-resident K = 512 rows above; "512 streamed" is the
    # same K through the streamed form.  `spread` = (max - min) / median of 5 repeats of the timed window.
    from vidar_amd.plugin.dense_heads.ray_ops import ray_dist, force_streamed
    import contextlib

    def rep(fn, n=5):
        ms = sorted(timeit(fn) for _ in range(n))
        return ms[n // 2], round((ms[-1] - ms[0]) / ms[n // 2], 3)
    R = pts.shape[0]
    for K, step, streamed in ((512, 1.0, False), (512, 1.0, True), (1026, 1.0, False), (1024, 0.5, False)):
        tag = f"K={K} step={step}" + (" streamed" if streamed else "")
        with (force_streamed() if streamed else contextlib.nullcontext()):
            ms, sp = rep(lambda: ray_ce(sigma, o, p, ti, step, K))
            report(f"ray_ce_fwd {tag}", ms, 4 * (16 * 200 * 200 + 30000 * 5), spread=sp)
            ce, valid = ray_ce(sigma, o, p, ti, step, K)
            ms, sp = rep(lambda: torch.autograd.grad(ce, sigma, g, retain_graph=True))
            report(f"ray_ce_bwd {tag}", ms, 4 * (2 * 16 * 200 * 200 + 30000 * 5), spread=sp)
            noise = gumbel_noise(R, K)
            ms, sp = rep(lambda: ray_gumbel(sigma, o, pts, tix, noise, step, K))
            report(f"ray_gumbel_fwd {tag}", ms, 4 * (16 * 200 * 200 + R * (K + 4)), spread=sp)
            d = ray_gumbel(sigma, o, pts, tix, noise, step, K)
            ms, sp = rep(lambda: torch.autograd.grad(d, sigma, torch.ones_like(d), retain_graph=True))
            report(f"ray_gumbel_bwd {tag}", ms, 4 * (2 * 16 * 200 * 200 + R * 4), spread=sp)
    # the distance loss on the GT rays of ray_ce (use_dist_loss), noise [30000, K + 1]
    for K, step in ((512, 1.0), (1024, 0.5)):
        noise = gumbel_noise(p.shape[0], K + 1)
        ms, sp = rep(lambda: ray_dist(sigma, o, p, ti, noise, step, K))
        report(f"ray_dist_fwd P=30000 K={K} step={step}", ms, 4 * (16 * 200 * 200 + 30000 * (K + 11)), spread=sp)
        dd, _, _ = ray_dist(sigma, o, p, ti, noise, step, K)
        ms, sp = rep(lambda: torch.autograd.grad(dd, sigma, g, retain_graph=True))
        report(f"ray_dist_bwd P=30000 K={K} step={step}", ms, 4 * (2 * 16 * 200 * 200 + 30000 * 8), spread=sp)


def bench_gemm(which):
    """the hot path's GEMM shapes: library (torch addmm / bmm, TunableOp off) vs csrc/gemm_mfma.hip in both modes.
    TF/s is the effective fp32-product rate 2MNK / time."""
    from vidar_amd import gemm as G
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g) * 2 - 1

    def line(name, flops, nbytes, **ms):
        d = {"op": name}
        for k, v in ms.items():
            d[k + "_ms"] = round(v, 4); d[k + "_TF"] = round(flops / v / 1e9, 1)
        d["min_HBM_ms"] = round(nbytes / 8e9, 4)
        print(json.dumps(d), flush=True)

    # nn.Linear shapes: value_proj (SCA), TSA offsets, FFN, output_proj
    for (M, K, N, tag) in ((184950, 256, 256, "value_proj SCA"), (80000, 256, 256, "value_proj TSA"),
                           (40000, 512, 128, "tsa sampling_offsets"), (40000, 256, 512, "ffn.0"),
                           (40000, 512, 256, "ffn.1"), (46080, 256, 512, "sca sampling_offsets")):
        x, w, b = rnd(M, K), rnd(N, K) * 0.1, rnd(N)
        gy = rnd(M, N)
        fl = 2.0 * M * N * K
        ms = dict(lib=timeit(lambda: torch.addmm(b, x, w.t())))
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.linear_forward(x, w, b, False, p))
        line(f"linear fwd [{M},{K}]x[{K},{N}] {tag}", fl, 4 * (M * K + M * N + N * K), **ms)
        ms = dict(lib=timeit(lambda: gy @ w))
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.linear_grad_input(gy, w, p))
        line(f"linear dx  [{M},{N}]x[{N},{K}] {tag}", fl, 4 * (M * K + M * N + N * K), **ms)
        ms = dict(lib=timeit(lambda: (x.t() @ gy).t()))
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.linear_grad_weight(gy, x, p))
        line(f"linear dw  [{N},{M}]x[{M},{K}] {tag}", fl, 4 * (M * K + M * N + N * K), **ms)
    # backbone: out[b] = W [Co,Ci] x[b] [Ci,HW]
    for (Bn, Co, Ci, HW, tag) in ((24, 1024, 256, 5800, "layer3 conv3"), (24, 256, 1024, 5800, "layer3 conv1"),
                                  (24, 256, 2304, 5800, "layer3 dcn"), (24, 512, 128, 23200, "layer2 conv3"),
                                  (24, 2048, 512, 1450, "layer4 conv3"), (24, 256, 64, 92800, "layer1 conv3")):
        w, x = rnd(Co, Ci) * 0.05, rnd(Bn, Ci, HW)
        sc, sh, res = rnd(Co), rnd(Co), rnd(Bn, Co, HW)
        fl = 2.0 * Bn * Co * Ci * HW
        nb = 4 * (Bn * Ci * HW + Bn * Co * HW)
        ms = dict(lib=timeit(lambda: torch.bmm(w.view(1, Co, Ci).expand(Bn, -1, -1), x)))
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.conv_forward(w, x, precision=p))
            ms[m + "_bn_res_relu"] = timeit(lambda: G.conv_forward(w, x, sc, sh, res, True, p))
        line(f"conv fwd {Bn}x[{Co},{Ci}]x[{Ci},{HW}] {tag}", fl, nb, **ms)
        gy = rnd(6, Co, HW); x6 = x[:6]
        fl6 = fl / 4
        ms = {}                                    # the 6 current images of a step (the 24 above are its history frames)
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.conv_forward(w, x6, precision=p))
            ms[m + "_bn_res_relu"] = timeit(lambda: G.conv_forward(w, x6, sc, sh, res[:6], True, p))
        line(f"conv fwd 6x[{Co},{Ci}]x[{Ci},{HW}] {tag}", fl6, nb / 4, **ms)
        ms = dict(lib=timeit(lambda: torch.bmm(w.view(1, Co, Ci).transpose(1, 2).expand(6, -1, -1), gy)))
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.conv_grad_input(w, gy, p))
        line(f"conv dx  6x[{Ci},{Co}]x[{Co},{HW}] {tag}", fl6, nb / 4, **ms)
        ms = dict(lib=timeit(lambda: torch.bmm(gy, x6.transpose(1, 2)).sum(0)))
        for m, p in (("f32", G.F32), ("bf16x3", G.BF16X3)):
            ms[m] = timeit(lambda: G.conv_grad_weight(gy, x6, p))
        line(f"conv dw  6x[{Co},{HW}]x[{HW},{Ci}] {tag}", fl6, nb / 4, **ms)


def bench_conv_offset(which):
    """the DCNv2 `conv_offset` (3x3, C -> 27) at the backbone's four cases: csrc/conv3x3_mfma.hip vs the library convolution"""
    import torch.nn.functional as F
    from vidar_amd.plugin.backbones import _Conv3x3Few
    torch.manual_seed(0)
    for (N, C, H, W) in [(24, 256, 58, 100), (6, 256, 58, 100), (24, 512, 29, 50), (6, 512, 29, 50)]:
        x = torch.randn(N, C, H, W, device="cuda")
        w = torch.randn(27, C, 3, 3, device="cuda") * 0.02
        b = torch.randn(27, device="cuda")
        flops = 2 * 27 * C * 9 * N * H * W
        with torch.no_grad():
            ref = F.conv2d(x, w, b, padding=1)
            got = _Conv3x3Few.apply(x, w, b)
            err = float((got - ref).abs().max() / ref.abs().max())
            ms_lib = timeit(lambda: F.conv2d(x, w, b, padding=1))
            ms_own = timeit(lambda: _Conv3x3Few.apply(x, w, b))
        report(f"conv_offset[{N},{C},{H},{W}] own", ms_own, 4 * (x.numel() + got.numel()), TFLOPs=round(flops / ms_own / 1e9, 1),
               frac_fp32_mfma=round(flops * 32 / 27 / ms_own / 1e9 / 157.3, 3), rel_err_vs_lib=err)
        report(f"conv_offset[{N},{C},{H},{W}] library", ms_lib, 4 * (x.numel() + got.numel()), TFLOPs=round(flops / ms_lib / 1e9, 1))


def bench_gemm_pmc(which):
    """a few launches of the representative GEMM shapes per mode, for the counter passes (tools/pmc_pass.sh)"""
    from vidar_amd import gemm as G
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g) * 2 - 1
    x, w, b = rnd(184950, 256), rnd(256, 256) * 0.1, rnd(256)
    wc, xc = rnd(1024, 256) * 0.05, rnd(24, 256, 5800)
    for p in (G.F32, G.BF16X3):
        for _ in range(3):
            G.linear_forward(x, w, b, False, p)
            G.conv_forward(wc, xc, precision=p)
    torch.cuda.synchronize()


def det_operands(seed, NL, B, Q, C, counts, device):
    """synthetic operands of the detection loss tail: logits, box codes, packed normalised ground truth"""
    from vidar_amd.plugin.core_bbox import normalize_bbox
    from vidar_amd.plugin.dense_heads import det_ops
    from vidar_amd.synthetic import boxes_3d
    g = torch.Generator().manual_seed(seed)
    cls = (torch.randn(NL, B, Q, C, generator=g) * 2 - 3).to(device)
    box = torch.randn(NL, B, Q, 10, generator=g).to(device)
    bl = [boxes_3d(seed + b, num=n) for b, n in enumerate(counts)]
    raw = torch.from_numpy(np.concatenate([b for b, _ in bl])).to(device)
    raw = torch.cat([raw[:, :2], raw[:, 2:3] + raw[:, 5:6] * 0.5, raw[:, 3:]], 1)
    gt_norm = normalize_bbox(raw) if raw.shape[0] else torch.zeros((0, 10), device=device)
    gt_label = torch.from_numpy(np.concatenate([l for _, l in bl])).to(device=device, dtype=torch.int32)
    gt_start = torch.from_numpy(det_ops.gt_starts(counts)).to(device)
    cw = torch.tensor([1.0] * 8 + [0.2] * 2, device=device)
    return cls, box, gt_norm.contiguous(), gt_label, gt_start, cw


def bench_det(which):
    """the detection loss tail of one fine-tune step (NL 6, B 1, Q 900, C 10): fused HIP kernels against the plain PyTorch
    composition of the same arithmetic, same process.  Device time per piece by HIP events (median of 5 x 50), and the
    whole tail -- cost, assignment, losses forward + backward -- by wall clock with a device drain (median of 30), with
    the assignment on the host (the default) and on the device (csrc/det_assign.hip).  The assignment alone: the host path
    (pinned copy, wait, SciPy over the 6 problems, upload) by wall clock with a device drain, the device launch by HIP
    events; the assignments of the two are compared before anything is timed."""
    import time
    from vidar_amd.plugin.dense_heads import det_ops as D
    dev = torch.device("cuda", 0)
    NL, B, Q, C = 6, 1, 900, 10
    for G in (37, 150, 512):
        counts = [G]
        cls, box, gt_norm, gt_label, gt_start, cw = det_operands(G, NL, B, Q, C, counts, dev)
        cls.requires_grad_(True); box.requires_grad_(True)
        args = (0.25, 2.0, 2.0, 0.25)
        matched = D.hungarian(D.match_cost(cls, box, gt_norm, gt_label, gt_start, G, *args), NL, Q, counts)
        labels = D.labels_from_matched(matched, gt_label, gt_start, C)
        gsum = torch.ones(NL, 2, device=dev)

        def loss_pair(fn):
            s = fn(cls, box, labels, matched, gt_norm, gt_start, cw, 0.25, 2.0)
            torch.autograd.grad(s, [cls, box], gsum)

        cost0 = D.match_cost(cls, box, gt_norm, gt_label, gt_start, G, *args)
        m_dev, st_dev = D.assign_device(cost0, NL, B, Q, gt_start, G)
        assert torch.equal(m_dev, matched) and not bool(st_dev.any()), "device and host assignments differ"

        def tail(fused, device_assign=False):
            cost = (D.match_cost(cls, box, gt_norm, gt_label, gt_start, G, *args) if fused
                    else D.match_cost_torch(cls.detach(), box.detach(), gt_norm, gt_label, counts, *args))
            m = D.assign_device(cost, NL, B, Q, gt_start, G)[0] if device_assign else D.hungarian(cost, NL, Q, counts)
            lab = D.labels_from_matched(m, gt_label, gt_start, C)
            s = (D.DetLossFunction.apply if fused else D.det_loss_sums_torch)(cls, box, lab, m, gt_norm, gt_start, cw, 0.25, 2.0)
            torch.autograd.grad(s, [cls, box], gsum)

        med = lambda f: float(np.median([timeit(f, warm=5, it=50) for _ in range(5)]))
        r = dict(G=G,
                 cost_hip_ms=med(lambda: D.match_cost(cls, box, gt_norm, gt_label, gt_start, G, *args)),
                 cost_torch_ms=med(lambda: D.match_cost_torch(cls.detach(), box.detach(), gt_norm, gt_label, counts, *args)),
                 loss_fwd_bwd_hip_ms=med(lambda: loss_pair(D.DetLossFunction.apply)),
                 loss_fwd_bwd_torch_ms=med(lambda: loss_pair(D.det_loss_sums_torch)))
        r["assign_device_ms"] = float(np.median([timeit(lambda: D.assign_device(cost0, NL, B, Q, gt_start, G), warm=3, it=20)
                                                 for _ in range(5)]))

        def wall(f):
            ts = []
            for i in range(35):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts[5:]))
        r["assign_host_wall_ms"] = wall(lambda: D.hungarian(cost0, NL, Q, counts))
        r["assign_device_wall_ms"] = wall(lambda: D.assign_device(cost0, NL, B, Q, gt_start, G))
        r["tail_wall_hip_ms"] = wall(lambda: tail(True))
        r["tail_wall_hip_device_assign_ms"] = wall(lambda: tail(True, True))
        r["tail_wall_torch_ms"] = wall(lambda: tail(False))
        report("det_loss_tail", r.pop("loss_fwd_bwd_hip_ms"), **{k: round(v, 4) if isinstance(v, float) else v for k, v in r.items()})


def det_eval_operands(seed, samples, preds_per_sample=300, mean_gt=30, device="cpu"):
    """synthetic detections at validation-split scale: per sample ~mean_gt annotations (Poisson) anywhere within 50 m and
    preds_per_sample predictions, 60 % of them scattered (sigma 1 m) around an annotation of their class, the rest
    anywhere; distinct random scores.  -> (pred, gt) lists of per-sample dicts of tensors on `device`"""
    rng = np.random.default_rng(seed)
    pred, gt = [], []
    for _ in range(samples):
        G = int(rng.poisson(mean_gt))
        gl = rng.integers(0, 10, G)
        gb = np.concatenate([rng.uniform(-50, 50, (G, 2)), rng.uniform(-2, 0, (G, 1)), rng.uniform(0.4, 10, (G, 3)),
                             rng.uniform(-np.pi, np.pi, (G, 1)), rng.normal(0, 2, (G, 2))], 1)
        P = preds_per_sample
        pl = rng.integers(0, 10, P)
        pb = np.concatenate([rng.uniform(-50, 50, (P, 2)), rng.uniform(-2, 0, (P, 1)), rng.uniform(0.4, 10, (P, 3)),
                             rng.uniform(-np.pi, np.pi, (P, 1)), rng.normal(0, 2, (P, 2))], 1)
        if G:
            near = rng.uniform(0, 1, P) < 0.6
            src = rng.integers(0, G, P)
            pb[near] = gb[src[near]] + rng.normal(0, 1.0, (int(near.sum()), 9)) * [1, 1, .1, .1, .1, .1, .1, .5, .5]
            pl[near] = gl[src[near]]
        pred.append(dict(boxes=pb.astype(np.float32), scores=rng.uniform(0.01, 1, P).astype(np.float32), labels=pl.astype(np.int64)))
        gt.append(dict(boxes=gb.astype(np.float32), labels=gl.astype(np.int64), num_pts=rng.integers(0, 40, G).astype(np.int64)))
    to = lambda side: [{k: torch.from_numpy(v).to(device) for k, v in s.items()} for s in side]
    return (pred, gt) if device == "cpu" else (to(pred), to(gt))


def bench_det_eval(which):
    """the detection metric at validation-split scale on synthetic boxes (6019 samples x 300 predictions, ~30 annotations
    each): the matcher launch alone by HIP events (median of 5 x 10), the torch plumbing in front of it and the whole
    DetectionEval.evaluate by wall clock with a device drain (median of 5).  Next to it the loops of the test suite's
    restatement of the devkit (tests/det_eval_cases.py -- only timed here, nothing is compared) on the host for a 1/50
    slice of the samples, and that time scaled by 50."""
    import time
    from vidar_amd.det_evaluate import DetectionEval
    dev = torch.device("cuda", 0)
    S = 6019
    host_pred, host_gt = det_eval_operands(0, S)
    to = lambda side: [{k: torch.from_numpy(v).to(dev) for k, v in s.items()} for s in side]
    pred, gt = to(host_pred), to(host_gt)
    ev = DetectionEval()

    def wall(fn, n=5):
        ts = []
        for _ in range(n + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:]))
    k = ev.prepare(pred, gt)
    P, G = k["pred_box"].shape[0], k["gt_box"].shape[0]
    kernel_ms = float(np.median([timeit(lambda: ev.run_matcher(k), warm=2, it=10) for _ in range(5)]))
    prepare_ms, evaluate_ms = wall(lambda: ev.prepare(pred, gt)), wall(lambda: ev.evaluate(pred, gt))
    result = ev.evaluate(pred, gt)
    sys.path.insert(0, str(ROOT / "tests"))
    import det_eval_cases                                       # the host loops, for the time only
    n = S // 50
    t0 = time.perf_counter()
    host = det_eval_cases.evaluate(dict(pred=host_pred[:n], gt=host_gt[:n]))
    host_s = time.perf_counter() - t0
    report("det_eval", kernel_ms, 36 * (P + G) + 4 * (4 * P + 4 * G) + 20 * P, samples=S, predictions=P, annotations=G,
           segments=k["NS"], thresholds=4, prepare_wall_ms=round(prepare_ms, 2), evaluate_wall_ms=round(evaluate_ms, 2),
           mAP=round(result["mean_ap"], 4), NDS=round(result["nd_score"], 4), host_loops_samples=n,
           host_loops_s=round(host_s, 2), host_loops_scaled_to_split_s=round(host_s * S / n, 1),
           host_slice_mAP=round(host["mean_ap"], 4))


def ray_eval_operands(seed, bs=1, frames=4, rays=30000, device="cpu"):
    """rays of a forecast as dense_heads get_rendered_rays hands them over: [bs, frames * rays] rendered points of the
    predicted and of the ground-truth depth (the prediction on the ground-truth ray, 0.7 .. 1.3 of its depth), the frame
    of every ray (2 % take no part: -1) and one origin per (sample, frame)"""
    rng = np.random.default_rng(seed)
    N = frames * rays
    origin = rng.uniform(-2, 2, (bs, frames, 3)) * [1, 1, 0.2]
    frame = np.tile(np.repeat(np.arange(frames), rays), (bs, 1))
    o = np.take_along_axis(origin, frame[..., None].repeat(3, -1), 1)
    end = rng.uniform(-90, 90, (bs, N, 3)) * [1, 1, 0.06]
    unit = (end - o) / np.linalg.norm(end - o, axis=-1, keepdims=True)
    depth = np.linalg.norm(end - o, axis=-1, keepdims=True)
    gt, pred = o + unit * depth, o + unit * depth * rng.uniform(0.7, 1.3, (bs, N, 1))
    frame = np.where(rng.uniform(size=(bs, N)) < 0.02, -1, frame)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)
    return t(pred, torch.float32), t(gt, torch.float32), t(frame, torch.int64), t(origin, torch.float32)


def bench_ray_eval(which):
    """the forecasting metric tail of ViDAR.forward_test for 4 segments x 30 000 rays (one sample, current + 3 future
    frames): the host path as forward_test runs it (boolean selection, chamfer through the KNN kernel, numpy ray errors
    with the nearest neighbour on the KNN kernel, a float() per figure) against eval_utils.forecast_metrics_device plus
    its one host read, both by wall clock with a device drain (median of 5 after one warm-up); and the two ray-error
    launches alone by HIP events.  Writes profiles/kbench_ray_eval.md."""
    import time
    from vidar_amd.plugin.utils import e2e_predictor_utils as E
    from vidar_amd.plugin.utils import eval_utils as U
    dev = torch.device("cuda", 0)
    pc_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    bs, F_, R = 1, 4, 30000
    pred, gt, frame, origin = ray_eval_operands(0, bs, F_, R, dev)

    def host_tail():
        out = np.zeros((bs, F_, 3))
        for b in range(bs):
            for f in range(F_):
                m = frame[b] == f
                p, g = pred[b][m], gt[b][m]
                cd = float(E.compute_chamfer_distance_inner(p, g, pc_range))
                l1, ar = U.compute_ray_errors(p.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64),
                                              origin[b, f].cpu().numpy().astype(np.float64), p.device)
                out[b, f] = cd, float(l1), float(ar)
        return out

    def device_tail():
        return U.forecast_metrics_device(pred, gt, frame, origin, pc_range).cpu().numpy()[..., :3]

    def wall(fn, n=5):
        ts = []
        for _ in range(n + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[1:])), ts[1:]
    device_ms, device_all = wall(device_tail)
    host_ms, host_all = wall(host_tail)
    h, d = host_tail(), device_tail()
    # the ray-error launches alone, on operands already in segment order
    S, N = bs * F_, frame.shape[1]
    key, order = torch.sort(torch.where(frame >= 0, frame, torch.full_like(frame, S)).reshape(-1), stable=True)
    start = torch.searchsorted(key, torch.arange(S + 1, device=dev)).to(torch.int32)
    sp, sg, so = pred.reshape(-1, 3)[order], gt.reshape(-1, 3)[order], origin.reshape(S, 3)
    kernel_ms = float(np.median([timeit(lambda: U.ray_errors_device(sp, start, sg, start, so, N), warm=2, it=10)
                                 for _ in range(5)]))
    row = dict(segments=S, rays_per_segment=R, ray_error_launches_ms=round(kernel_ms, 3), device_tail_wall_ms=round(device_ms, 2),
               host_tail_wall_ms=round(host_ms, 2), host_over_device=round(host_ms / device_ms, 1),
               device_runs_ms=[round(t, 2) for t in device_all], host_runs_ms=[round(t, 2) for t in host_all],
               max_rel_diff_chamfer=float(np.abs(d[..., 0] / h[..., 0] - 1).max()),
               max_rel_diff_l1=float(np.abs(d[..., 1] / h[..., 1] - 1).max()),
               max_rel_diff_absrel=float(np.abs(d[..., 2] / h[..., 2] - 1).max()))
    report("ray_eval", kernel_ms, **row)
    (ROOT / "profiles" / "kbench_ray_eval.md").write_text(
        "# Forecasting metric tail on an MI355X: `python tools/kbench.py ray_eval`\n\n"
        f"{S} segments (1 sample, current + 3 future frames) x {R} rays, 2 % of the rays dropped; the prediction sits on the\n"
        "ground-truth ray at 0.7 .. 1.3 of its depth (`tools/kbench.py::ray_eval_operands`).  Wall clock with a device drain,\n"
        "median of 5 after one warm-up; the two ray-error launches alone by HIP events (median of 5 x 10).\n\n"
        "```\n" + json.dumps({"device": torch.cuda.get_device_name(0)}) + "\n" + json.dumps(dict(op="ray_eval", **row)) + "\n```\n\n"
        "| what | result |\n|---|---|\n"
        f"| host tail of `ViDAR.forward_test` (selection, chamfer, numpy ray errors, a `float()` per figure) | {host_ms:.2f} ms |\n"
        f"| device tail (`eval_utils.forecast_metrics_device` and its one host read) | {device_ms:.2f} ms |\n"
        f"| `vidar_ray_eval_f64` (projection + match launches) alone | {kernel_ms:.3f} ms |\n\n"
        "The `max_rel_diff_*` figures compare the two tails' results on these operands; they are printed to show that both\n"
        "sides computed the same thing (the host path searches the nearest neighbour in fp32, the device path in fp64).\n")


def bench_deterministic(which):
    """every backward the deterministic mode covers (vidar_amd/deterministic.py) at its BASELINE shape, in both modes:
    mode=0 the fp32-atomic default (with the strategy the step takes), mode=1 the measure + fixed-point (or fixed-order)
    form.  `det` is the detection-loss bench, hence the long name."""
    from vidar_amd import deterministic, gemm
    from vidar_amd.synthetic import msda_operands, ray_set, dense_rays
    from vidar_amd.plugin.modules.multi_scale_deformable_attn_function import _msda_backward
    from vidar_amd.plugin.dense_heads.ray_ops import ray_ce, ray_gumbel, ray_dist, gumbel_noise
    from vidar_amd.plugin.modules.ray_operations.latent_rendering import _PathProb, _RayGather
    from vidar_amd.plugin.backbones import dcn_col2im
    from vidar_amd.plugin.bricks import drop_add_layernorm
    from vidar_amd.third_lib.chamferdist import _C
    import torch.nn as nn
    cases = []
    fpn = [(116, 200), (58, 100), (29, 50), (15, 25)]
    for name, B, shapes, Nq, P in (("TSA", 2, [(200, 200)], 40000, 4), ("SCA", 6, fpn, 10000, 8)):
        value, sh, lsi, loc, w = msda_operands(0, B, shapes, Nq, P=P, device="cuda")
        go = torch.randn(B, Nq, 256, device="cuda")
        cases.append((f"msda_bwd {name}", lambda a=(value, sh, lsi, loc, w, go): _msda_backward(*a)))
    sig, origin, points, tindex = ray_set(seed=0, N=1, T=1, rays_per_frame=30000)
    sigma = torch.randn(1, 16, 200, 200, device="cuda", requires_grad=True)
    o, p, ti = (torch.from_numpy(a[0]).cuda() for a in (origin, points, tindex))
    pts, tix = dense_rays(1, 16, 200, 200, "cuda")
    ce, _ = ray_ce(sigma, o, p, ti)
    dg = ray_gumbel(sigma, o, pts, tix, gumbel_noise(pts.shape[0], 512))
    dd, _, _ = ray_dist(sigma, o, p, ti, gumbel_noise(p.shape[0], 513))
    for name, q in (("ray_ce_bwd P=30000", ce), (f"ray_gumbel_bwd R={pts.shape[0]}", dg), ("ray_dist_bwd P=30000", dd)):
        cases.append((name, lambda q=q, g=torch.ones_like(q): torch.autograd.grad(q, sigma, g, retain_graph=True)))
    occ = torch.randn(1, 200, 200, 16, device="cuda", requires_grad=True)
    a = torch.randn(1, 200, 200, 16, device="cuda", requires_grad=True)
    pr = _PathProb.apply(occ, 256, 1.0, 0)
    pd = pr.detach().requires_grad_(True)
    f = _RayGather.apply(pd, a, 256, 1.0, 1e-3)
    cases.append(("lr_prob_bwd step=1.0", lambda g=torch.randn_like(pr): torch.autograd.grad(pr, occ, g, retain_graph=True)))
    cases.append(("lr_gather_bwd step=1.0", lambda g=torch.randn_like(f): torch.autograd.grad(f, [pd, a], g, retain_graph=True)))
    rng = np.random.default_rng(0)
    c1 = torch.from_numpy(rng.uniform(-50, 50, (1, 30000, 3)).astype(np.float32)).cuda()
    c2 = torch.from_numpy(rng.uniform(-50, 50, (1, 30000, 3)).astype(np.float32)).cuda()
    l = torch.tensor([30000], device="cuda")
    idx, _ = _C.knn_points_idx(c1, c2, l, l, 1, -1)
    gd = torch.randn(1, 30000, 1, device="cuda")
    cases.append(("knn1_d3_bwd 30000x30000", lambda: _C.knn_points_backward(c1, c2, l, l, idx, gd)))
    g = torch.Generator().manual_seed(0)
    N, C, H, W = 6, 256, 58, 100
    x = torch.randn(N, C, H, W, generator=g).cuda(); mask = torch.rand(N, 9, H, W, generator=g).cuda()
    gcols = torch.randn(N, C * 9, H * W, generator=g).cuda(); off = (torch.randn(N, 18, H, W, generator=g) * 1.5).cuda()
    cases.append((f"dcn_col2im N={N} C={C} {H}x{W} offsets~1.5px", lambda: dcn_col2im(gcols, x, off, mask, 3, 3, 1, 1, 1, H, W)))
    norm = nn.LayerNorm(256).cuda()
    xs = torch.randn(1, 40000, 256, device="cuda", requires_grad=True); rs = torch.randn(1, 40000, 256, device="cuda", requires_grad=True)
    y = drop_add_layernorm(xs, rs, norm, 0.1, True)
    cases.append(("drop_add_ln bwd", lambda gy=torch.randn_like(y): torch.autograd.grad(y, [xs, rs, norm.weight, norm.bias], gy, retain_graph=True)))
    g2 = torch.randn(40000, 256, device="cuda")
    cases.append(("colsum 40000x256", lambda: gemm._colsum(g2)))
    for name, fn in cases:
        for mode in (False, True):
            with deterministic.use(mode):
                ms = sorted(timeit(fn) for _ in range(3))[1]
            report(name, ms, mode=int(mode))


def bench_imgprep(which):
    """the device image pipeline on one sample (30 images of 900 x 1600, random noise) for the three released pipelines,
    against the host path (numpy / PIL / torch, this process, its torch threads) on the same images and the same drawn
    parameters.  Device ms by HIP events (median of 5 x 10); modelled bytes = uint8 in + fp32 out + the uint8 intermediates
    the kernels actually write and read back.  JPEG decode is not part of either side."""
    import random
    import time
    from vidar_amd.data.augment import CropResizeFlipImage, PhotoMetricDistortionMultiViewImage
    from vidar_amd.data.device_prep import DeviceImagePrep, host_prep, out_shape
    n, H, W = 30, 900, 1600
    raw = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, H, W, 3), dtype=np.uint8))
    dev_raw = raw.cuda()
    prep = DeviceImagePrep()
    np.random.seed(0); random.seed(0)
    photo = PhotoMetricDistortionMultiViewImage().draw(n)
    _, dims, crop, flip = CropResizeFlipImage().sample({})
    plans = {"nuscenes_train": dict(photo=photo, resize_dims=dims, crop=crop, flip=flip, img_scale=None),
             "nuscenes_test": dict(photo=None, resize_dims=None, crop=None, flip=False, img_scale=None),
             "openscene_train": dict(photo=photo, resize_dims=None, crop=None, flip=False, img_scale=2.0 / 3.0)}
    for name, plan in plans.items():
        out = prep(dev_raw, plan)
        oh, ow = out_shape(plan, H, W)
        nbytes = raw.numel() + out.numel() * 4
        if plan["resize_dims"] is not None:
            nbytes += 2 * raw.numel()                                 # photometric: uint8 plane written, read by the resample
            if (ow, oh) != (W, H) or plan["flip"]:
                nbytes += 2 * n * H * ow * 3 * (oh != H)              # horizontal pass' plane, when a vertical pass follows
                nbytes += 2 * n * oh * ow * 3                         # resampled plane written, read by the normalise
        ms = float(np.median([timeit(lambda: prep(dev_raw, plan), warm=2, it=10) for _ in range(5)]))
        k = 2 if name == "nuscenes_train" else 6                      # host: a few images, scaled to the sample
        t0 = time.perf_counter()
        host_prep(raw[:k].numpy(), dict(plan, photo=None if plan["photo"] is None else plan["photo"][:k]), prep.mean, prep.std,
                  prep.to_rgb, prep.size_divisor)
        host_ms = (time.perf_counter() - t0) * 1e3 * n / k
        report("imgprep_" + name, ms, nbytes, images=n, out_shape=list(out.shape), host_ms_per_sample=round(host_ms, 1),
               host_images_timed=k, host_threads=torch.get_num_threads())


def bench_forecast_view(which):
    """the camera-view decode of one predicted frame at 200 x 200 x 16, K = 512, step 1: 6 cameras of 900 x 1600 pixels at
    strides 1 / 2 / 4, the fused entry (vidar_ray_argmax_cam_f32: the rays are never stored) against the materialised
    route (vidar_cam_rays_f32, then vidar_ray_argmax_f32 once per camera) in the same process on the same build.  HIP
    events, the two routes alternating, three repeats of 2 warm-up + 5 timed calls each; the spread is (max - min) /
    median over the repeats.  Writes profiles/kbench_forecast_view.md."""
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads.ray_ops import cam_rays, ray_argmax, ray_argmax_cam
    from vidar_amd.synthetic import PC_RANGE, camera_matrices
    dev = torch.device("cuda", 0)
    Z, Y, X, C, H, W, K = 16, 200, 200, 6, 900, 1600, 512
    sigma = torch.randn(1, Z, Y, X, generator=torch.Generator().manual_seed(0)).to(dev)
    m = FC.pix2vox(camera_matrices(img_hw=(H, W))[:C], PC_RANGE, Y, X, Z).to(dev)
    rows = []
    for stride in (1, 2, 4):
        Hs, Ws = -(-H // stride), -(-W // stride)
        geom = ((Hs, Ws), stride / 2.0, stride / 2.0, float(stride), float(stride))
        tindex = torch.zeros(Hs * Ws, device=dev)

        def fused():
            return ray_argmax_cam(sigma, m, *geom, 1.0, K)

        def two_launch():
            origin, pts = cam_rays(m, *geom)
            return [ray_argmax(sigma, origin[:, c].contiguous(), pts[0, c].reshape(-1, 3), tindex, 1.0, K)[0]
                    for c in range(C)]
        a, b = fused(), torch.stack(two_launch()).view(1, C, Hs, Ws)
        live = a != 0
        same = bool(torch.equal(a[live], b[live]))
        fs, ts = [], []
        for _ in range(3):
            fs.append(timeit(fused, warm=2, it=5)); ts.append(timeit(two_launch, warm=2, it=5))
        med = lambda v: float(np.median(v))
        spread = lambda v: (max(v) - min(v)) / med(v)
        rays = C * Hs * Ws
        row = dict(stride=stride, rays=rays, ray_bytes_MB=round(rays * 12 / 1e6, 1), fused_ms=[round(v, 3) for v in fs],
                   two_launch_ms=[round(v, 3) for v in ts], fused_median_ms=round(med(fs), 3),
                   two_launch_median_ms=round(med(ts), 3), fused_spread=round(spread(fs), 4),
                   two_launch_spread=round(spread(ts), 4), fused_over_two_launch=round(med(fs) / med(ts), 4),
                   live_rays=int(live.sum()), same_bits_on_live_rays=same)
        rows.append(row)
        report("forecast_view", med(fs), **row)
    out = os.environ.get("VIDAR_KBENCH_OUT")
    path = Path(out) if out else ROOT / "profiles" / "kbench_forecast_view.md"
    path.write_text(
        "# Camera-view decode on an MI355X: `python tools/kbench.py forecast_view`\n\n"
        f"One predicted frame, volume {Z} x {Y} x {X}, K = {K}, step 1, {C} cameras of {H} x {W} pixels (the pin-hole rig of\n"
        "`vidar_amd.synthetic.camera_matrices`), random-normal logits.  `fused`: `vidar_ray_argmax_cam_f32`;\n"
        "`two_launch`: `vidar_cam_rays_f32` + `vidar_ray_argmax_f32` per camera (7 launches, the rays written and read back).\n"
        "HIP events, the routes alternating, 3 repeats of 2 warm-up + 5 timed calls; spread = (max - min) / median.\n\n"
        "```\n" + json.dumps({"device": torch.cuda.get_device_name(0)}) + "\n"
        + "\n".join(json.dumps(dict(op="forecast_view", **r)) for r in rows) + "\n```\n\n"
        "| stride | rays | rays as [R,3] fp32 | fused ms (median) | two-launch ms (median) | fused / two-launch | spread fused | spread two-launch |\n"
        "|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['stride']} | {r['rays']} | {r['ray_bytes_MB']} MB | {r['fused_median_ms']} | {r['two_launch_median_ms']} | "
                  f"{r['fused_over_two_launch']} | {r['fused_spread']} | {r['two_launch_spread']} |\n" for r in rows))


def bench_ray_stats(which):
    """the decode with its confidence (vidar_ray_stats_f32 / vidar_ray_stats_cam_f32) against the plain arg-max decode
    (vidar_ray_argmax_f32 / vidar_ray_argmax_cam_f32) in the same process on the same build: 30 000 listed rays, and 6
    cameras of 900 x 1600 pixels at strides 1 / 2 / 4, on a 16 x 200 x 200 volume at K = 512 (register form) and K = 1026
    (streamed form), step 1.  HIP events, the two decodes alternating, three repeats of 2 warm-up + 5 timed calls each
    (50 for the listed rays); the spread is (max - min) / median over the repeats.  Writes profiles/kbench_ray_stats.md."""
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads.ray_ops import ray_argmax, ray_argmax_cam, ray_stats, ray_stats_cam
    from vidar_amd.synthetic import PC_RANGE, camera_matrices, ray_set
    dev = torch.device("cuda", 0)
    Z, Y, X, C, H, W = 16, 200, 200, 6, 900, 1600
    sigma = torch.randn(1, Z, Y, X, generator=torch.Generator().manual_seed(0)).to(dev)
    _, origin, points, tindex = ray_set(seed=0, N=1, T=1, rays_per_frame=30000)
    o, p, ti = (torch.from_numpy(a[0]).to(dev) for a in (origin, points, tindex))
    m = FC.pix2vox(camera_matrices(img_hw=(H, W))[:C], PC_RANGE, Y, X, Z).to(dev)
    med = lambda v: float(np.median(v))
    spread = lambda v: (max(v) - min(v)) / med(v)
    rows = []

    def compare(rays, K, plain, stats, it=5, **tag):
        a, b = plain(), stats()
        same = bool(torch.equal(a, b[0]))
        ps, ss = [], []
        for _ in range(3):
            ps.append(timeit(plain, warm=2, it=it)); ss.append(timeit(stats, warm=2, it=it))
        row = dict(rays=tag.pop("rays_name"), **tag, R=rays, K=K, form="register" if K == 512 else "streamed",
                   argmax_ms=[round(v, 3) for v in ps], stats_ms=[round(v, 3) for v in ss],
                   argmax_median_ms=round(med(ps), 3), stats_median_ms=round(med(ss), 3),
                   argmax_spread=round(spread(ps), 4), stats_spread=round(spread(ss), 4),
                   stats_over_argmax=round(med(ss) / med(ps), 4), same_distance_bits=same,
                   mean_p_max=round(float(b[-1][..., 0].mean()), 4))
        rows.append(row)
        report("ray_stats", med(ss), **row)

    for K in (512, 1026):
        compare(p.shape[0], K, lambda: ray_argmax(sigma, o, p, ti, 1.0, K)[0], lambda: ray_stats(sigma, o, p, ti, 1.0, K),
                it=50, rays_name="listed", stride="-")
    for K in (512, 1026):
        for stride in (1, 2, 4):
            Hs, Ws = -(-H // stride), -(-W // stride)
            geom = ((Hs, Ws), stride / 2.0, stride / 2.0, float(stride), float(stride))
            compare(C * Hs * Ws, K, lambda: ray_argmax_cam(sigma, m, *geom, 1.0, K),
                    lambda: ray_stats_cam(sigma, m, *geom, 1.0, K), rays_name="camera", stride=stride)
    out = os.environ.get("VIDAR_KBENCH_OUT")
    path = Path(out) if out else ROOT / "profiles" / "kbench_ray_stats.md"
    path.write_text(
        "# The decode with its confidence on an MI355X: `python tools/kbench.py ray_stats`\n\n"
        f"Volume {Z} x {Y} x {X}, random-normal logits, step 1.  `listed`: 30 000 rays of `vidar_amd.synthetic.ray_set`\n"
        f"(`vidar_ray_stats_f32` against `vidar_ray_argmax_f32`); `camera`: {C} cameras of {H} x {W} pixels, the pin-hole rig of\n"
        "`vidar_amd.synthetic.camera_matrices` (`vidar_ray_stats_cam_f32` against `vidar_ray_argmax_cam_f32`).  K = 512 runs\n"
        "the register form, K = 1026 the streamed one.  Both decodes in one process on one build, alternating; HIP events,\n"
        "3 repeats of 2 warm-up + 5 timed calls (50 for the listed rays); spread = (max - min) / median.  Each call\n"
        "allocates its outputs.\n\n"
        "```\n" + json.dumps({"device": torch.cuda.get_device_name(0)}) + "\n"
        + "\n".join(json.dumps(dict(op="ray_stats", **r)) for r in rows) + "\n```\n\n"
        "| rays | stride | R | K | form | arg-max ms (median) | stats ms (median) | stats / arg-max | spread arg-max | spread stats |\n"
        "|---|---|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['rays']} | {r['stride']} | {r['R']} | {r['K']} | {r['form']} | {r['argmax_median_ms']} | "
                  f"{r['stats_median_ms']} | {r['stats_over_argmax']} | {r['argmax_spread']} | {r['stats_spread']} |\n"
                  for r in rows))


def bench_ray_occupancy(which):
    """occupancy evidence (vidar_ray_occupancy_f32 / vidar_ray_occupancy_cam_f32) on a 16 x 200 x 200 volume, step 1, at
    K = 512 (register form) and K = 1026 (streamed), default and deterministic mode: the 34 560 rays of
    vidar_amd.forecast.lidar_pattern() from the volume's centre, and 6 cameras of 900 x 1600 pixels at strides 4 and 8.
    In the same process each row stands next to ray_stats on the same rays (the march without the scatter) and, for the
    listed rays, the ray_ce backward (the same scatter pattern into one volume).  HIP events, the ops alternating, three
    repeats of 2 warm-up + 5 timed calls (20 for the listed rays); the spread is (max - min) / median over the repeats.
    Writes profiles/kbench_ray_occupancy.md."""
    from vidar_amd import deterministic
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads.ray_ops import (cam_rays, ray_ce, ray_occupancy, ray_occupancy_cam, ray_stats,
                                                      ray_stats_cam)
    from vidar_amd.synthetic import PC_RANGE, camera_matrices
    dev = torch.device("cuda", 0)
    Z, Y, X, C, H, W = 16, 200, 200, 6, 900, 1600
    sigma = torch.randn(1, Z, Y, X, generator=torch.Generator().manual_seed(0)).to(dev)
    o = torch.tensor([[X / 2.0, Y / 2.0, Z / 4.0]], device=dev)
    p = o + FC.lidar_pattern().to(dev)
    ti = torch.zeros(p.shape[0], device=dev)
    m = FC.pix2vox(camera_matrices(img_hw=(H, W))[:C], PC_RANGE, Y, X, Z).to(dev)
    size = torch.tensor([X, Y, Z], device=dev, dtype=torch.float32)
    med = lambda v: float(np.median(v))
    spread = lambda v: (max(v) - min(v)) / med(v)
    rows = []

    def live_waypoints(origin, pts, K):
        """waypoints with a corner inside the volume (random-normal logits: no sample is an exact zero)"""
        n = 0
        k = (torch.arange(K, device=dev, dtype=torch.float32) + 0.5).view(1, K, 1)
        for i in range(0, pts.shape[0], 32768):
            d = pts[i:i + 32768] - origin[i:i + 32768]
            d = d / d.norm(dim=1, keepdim=True)
            pix = origin[i:i + 32768, None] + d[:, None] * k - 0.5
            n += int(((pix > -1) & (pix < size)).all(-1).sum())
        return n

    def compare(R, K, det, live, occ, stats, ce_bwd=None, it=5, **tag):
        with deterministic.use(det):
            hit, free = occ()
            ts = {"occupancy": [], "ray_stats": [], "ray_ce_bwd": []}
            for _ in range(3):
                ts["occupancy"].append(timeit(occ, warm=2, it=it)); ts["ray_stats"].append(timeit(stats, warm=2, it=it))
                if ce_bwd is not None:
                    ts["ray_ce_bwd"].append(timeit(ce_bwd, warm=2, it=it))
        t = med(ts["occupancy"])
        row = dict(**tag, R=R, K=K, form="register" if K == 512 else "streamed", mode="deterministic" if det else "default",
                   occupancy_ms=[round(v, 3) for v in ts["occupancy"]], occupancy_median_ms=round(t, 3),
                   occupancy_spread=round(spread(ts["occupancy"]), 4), ray_stats_median_ms=round(med(ts["ray_stats"]), 3),
                   ray_stats_spread=round(spread(ts["ray_stats"]), 4),
                   ray_ce_bwd_median_ms=round(med(ts["ray_ce_bwd"]), 3) if ce_bwd else None,
                   ray_ce_bwd_spread=round(spread(ts["ray_ce_bwd"]), 4) if ce_bwd else None,
                   live_waypoints=live, atomic_adds=live * 16, giga_adds_per_s=round(live * 16 / t / 1e6, 1),
                   hit_sum=round(float(hit.sum()), 2), free_max=round(float(free.max()), 2))
        rows.append(row)
        report("ray_occupancy", t, **row)

    for K in (512, 1026):
        live = live_waypoints(o.expand(p.shape[0], 3), p, K)
        sg = sigma.clone().requires_grad_(True)
        for det in (False, True):
            with deterministic.use(det):
                ce, _ = ray_ce(sg, o, p, ti, 1.0, K)
            g = torch.ones_like(ce)
            compare(p.shape[0], K, det, live, lambda: ray_occupancy(sigma, o, p, ti, 1.0, K),
                    lambda: ray_stats(sigma, o, p, ti, 1.0, K),
                    lambda: torch.autograd.grad(ce, sg, g, retain_graph=True), it=20, rays="sweep", stride="-")
    for K in (512, 1026):
        for stride in (8, 4):
            Hs, Ws = -(-H // stride), -(-W // stride)
            geom = ((Hs, Ws), stride / 2.0, stride / 2.0, float(stride), float(stride))
            co, cp = cam_rays(m, *geom)
            live = live_waypoints(co[0, :, None, None].expand(C, Hs, Ws, 3).reshape(-1, 3), cp[0].reshape(-1, 3), K)
            del co, cp
            for det in (False, True):
                compare(C * Hs * Ws, K, det, live, lambda: ray_occupancy_cam(sigma, m, *geom, 1.0, K),
                        lambda: ray_stats_cam(sigma, m, *geom, 1.0, K), rays="camera", stride=stride)
    out = os.environ.get("VIDAR_KBENCH_OUT")
    path = Path(out) if out else ROOT / "profiles" / "kbench_ray_occupancy.md"
    cell = lambda v: "-" if v is None else v
    path.write_text(
        "# Occupancy evidence on an MI355X: `python tools/kbench.py ray_occupancy`\n\n"
        f"Volume {Z} x {Y} x {X}, random-normal logits, step 1.  `sweep`: the {p.shape[0]} rays of\n"
        f"`vidar_amd.forecast.lidar_pattern()` from the volume's centre (`vidar_ray_occupancy_f32`); `camera`: {C} cameras of\n"
        f"{H} x {W} pixels, the pin-hole rig of `vidar_amd.synthetic.camera_matrices` (`vidar_ray_occupancy_cam_f32`).  K = 512\n"
        "runs the register form, K = 1026 the streamed one; `default` adds with fp32 atomics into 8 private copies of both\n"
        "volumes, `deterministic` measures and then adds in 64-bit fixed point.  Next to each row, in the same process on the\n"
        "same rays: `ray_stats` (the march without the scatter) and, for the sweep, the `ray_ce` backward through autograd\n"
        "(the same scatter pattern into one volume).  HIP events, the ops alternating, 3 repeats of 2 warm-up + 5 timed calls\n"
        "(20 for the sweep); spread = (max - min) / median.  Each call allocates its outputs and its workspace.\n"
        "`atomic adds` = live waypoints x 8 corners x 2 volumes (an upper bound: corners outside the volume are dropped; the\n"
        "deterministic mode visits them twice, once to measure); `G adds / s` = that count over the median time.\n\n"
        "```\n" + json.dumps({"device": torch.cuda.get_device_name(0)}) + "\n"
        + "\n".join(json.dumps(dict(op="ray_occupancy", **r)) for r in rows) + "\n```\n\n"
        "| rays | stride | R | K | mode | occupancy ms (median) | spread | ray_stats ms | ray_ce_bwd ms | live waypoints | atomic adds | G adds / s |\n"
        "|---|---|---|---|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['rays']} | {r['stride']} | {r['R']} | {r['K']} | {r['mode']} | {r['occupancy_median_ms']} | "
                  f"{r['occupancy_spread']} | {r['ray_stats_median_ms']} | {cell(r['ray_ce_bwd_median_ms'])} | "
                  f"{r['live_waypoints']} | {r['atomic_adds']} | {r['giga_adds_per_s']} |\n" for r in rows))


def _occ_table_torch(pred, meas, thresholds, bins, min_pred=0.5, min_meas=0.5, min_hits=0.125):
    """forecast.occupancy_score's table as a torch program on the device (fp32 decisions, fp64 sums)"""
    hp, fp, hm, fm = pred[:, 0].flatten(1), pred[:, 1].flatten(1), meas[:, 0].flatten(1), meas[:, 1].flatten(1)
    finite = torch.isfinite(hp) & torch.isfinite(fp) & torch.isfinite(hm) & torch.isfinite(fm)
    ev_p, ev_m = hp + fp, hm + fm
    o_p = hp / ev_p
    ok_p, ok_m, y = finite & (ev_p >= min_pred), finite & (ev_m >= min_meas), hm >= min_hits
    both = ok_p & ok_m
    n = lambda m: m.sum(1, dtype=torch.float64)
    term = (o_p.double() - y.double()) ** 2
    cols = [n(ok_p), n(ok_m), n(both), n(both & y), torch.where(both, term, torch.zeros_like(term)).sum(1)]
    for t in thresholds:
        yhat = o_p >= t
        cols += [n(both & yhat & y), n(both & yhat & ~y), n(both & ~yhat & y)]
    b = (torch.where(both, o_p, torch.zeros_like(o_p)) * bins).long().clamp(max=bins - 1)
    for k in range(bins):
        cols += [n(both & (b == k)), n(both & (b == k) & y)]
    return torch.stack(cols, 1)


def bench_occ_score(which):
    """The occupancy score on a 16 x 200 x 200 volume, step 1.
    sweep_evidence (vidar_sweep_evidence_f32) next to ray_occupancy (vidar_ray_occupancy_f32) on the 34 560 rays of
    vidar_amd.forecast.lidar_pattern() from the volume's centre, end points 4 - 120 voxels out drawn from a seed; K = 512
    and 1026, default and deterministic mode, same process, the two ops alternating.
    occupancy_score (vidar_occ_score_f32, 2 thresholds, 10 bins) on those two grids for 1 and 7 segments, next to a torch
    program on the device that builds the same table and to a device copy of the same 16 B per voxel.
    HIP events, three repeats of 2 warm-up + 20 timed calls; spread = (max - min) / median.
    Writes profiles/kbench_occ_score.md."""
    from vidar_amd import deterministic
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads.ray_ops import ray_occupancy, sweep_evidence
    from vidar_amd._lib import lib, ptr, stream_of
    import ctypes
    dev = torch.device("cuda", 0)
    Z, Y, X = 16, 200, 200
    gen = torch.Generator().manual_seed(0)
    sigma = torch.randn(1, Z, Y, X, generator=gen).to(dev)
    o = torch.tensor([[X / 2.0, Y / 2.0, Z / 4.0]], device=dev)
    d = FC.lidar_pattern()
    length = 4.0 + 116.0 * torch.rand(d.shape[0], generator=gen)
    p = o + (d * length.view(-1, 1)).to(dev)
    ti = torch.zeros(p.shape[0], device=dev)
    med = lambda v: float(np.median(v))
    spread = lambda v: (max(v) - min(v)) / med(v)
    rows, score_rows = [], []
    grids = {}
    for K in (512, 1026):
        for det in (False, True):
            with deterministic.use(det):
                occ = lambda: ray_occupancy(sigma, o, p, ti, 1.0, K)
                swp = lambda: sweep_evidence(o, p, ti, sigma.shape, 1.0, K)
                grids[K] = (torch.stack(occ(), 1), torch.stack(swp(), 1))
                ts = {"sweep": [], "occupancy": []}
                for _ in range(3):
                    ts["sweep"].append(timeit(swp, warm=2, it=20)); ts["occupancy"].append(timeit(occ, warm=2, it=20))
            marched = int(torch.clamp(torch.ceil(length - 0.5), max=K).sum())
            row = dict(R=p.shape[0], K=K, mode="deterministic" if det else "default",
                       sweep_evidence_ms=[round(v, 3) for v in ts["sweep"]], sweep_evidence_median_ms=round(med(ts["sweep"]), 3),
                       sweep_evidence_spread=round(spread(ts["sweep"]), 4),
                       ray_occupancy_median_ms=round(med(ts["occupancy"]), 3),
                       ray_occupancy_spread=round(spread(ts["occupancy"]), 4),
                       ratio=round(med(ts["sweep"]) / med(ts["occupancy"]), 3), waypoints_with_a_weight=marched,
                       hit_sum=round(float(grids[K][1][:, 0].sum()), 2), free_max=round(float(grids[K][1][:, 1].max()), 2))
            rows.append(row)
            report("sweep_evidence", med(ts["sweep"]), **row)
    th, bins = (0.25, 0.5), 10
    for S in (1, 7):
        pred = grids[512][0].expand(S, 2, Z, Y, X).contiguous()
        meas = grids[512][1].expand(S, 2, Z, Y, X).contiguous()
        buf = torch.empty(2, *pred.shape, device=dev)
        kernel = lambda: FC.occupancy_score(pred, meas, thresholds=th, bins=bins)
        eager = lambda: _occ_table_torch(pred, meas, th, bins)
        copy = lambda: (buf[0].copy_(pred), buf[1].copy_(meas))
        # the entry point alone, on a table and a workspace allocated once: what the wrapper's allocations and Python cost
        nws = ctypes.c_int64(0)
        lib().vidar_occ_score_workspace_bytes(S, Z * Y * X, len(th), bins, ctypes.addressof(nws))
        table, ws = torch.empty(S, 5 + 3 * len(th) + 2 * bins, dtype=torch.float64, device=dev), torch.empty(nws.value, dtype=torch.uint8, device=dev)
        th_host, stream = (ctypes.c_float * len(th))(*th), stream_of(pred)
        entry = lambda: lib().vidar_occ_score_f32(ptr(pred), ptr(meas), ctypes.addressof(th_host), ptr(table), S, Z * Y * X,
                                                  len(th), bins, 0.5, 0.5, 0.125, ptr(ws), nws.value, stream)
        got, want = kernel(), eager()
        same = bool(torch.equal(got[:, [c for c in range(got.shape[1]) if c != 4]],
                                want[:, [c for c in range(got.shape[1]) if c != 4]]))
        assert entry() == 0 and torch.equal(table, got)
        ts = {"kernel": [], "entry": [], "torch": [], "copy": []}
        for _ in range(3):
            for name, fn in (("kernel", kernel), ("entry", entry), ("torch", eager), ("copy", copy)):
                ts[name].append(timeit(fn, warm=2, it=20))
        nbytes = 16 * S * Z * Y * X
        row = dict(S=S, V=Z * Y * X, T=len(th), B=bins, read_MB=round(nbytes / 1e6, 2),
                   kernel_ms=[round(v, 4) for v in ts["kernel"]], kernel_median_ms=round(med(ts["kernel"]), 4),
                   kernel_spread=round(spread(ts["kernel"]), 4), entry_median_ms=round(med(ts["entry"]), 4),
                   entry_spread=round(spread(ts["entry"]), 4), entry_GBps=round(nbytes / med(ts["entry"]) / 1e6, 1),
                   torch_median_ms=round(med(ts["torch"]), 3), torch_spread=round(spread(ts["torch"]), 4),
                   copy_median_ms=round(med(ts["copy"]), 4), copy_spread=round(spread(ts["copy"]), 4),
                   kernel_over_copy=round(med(ts["kernel"]) / med(ts["copy"]), 2),
                   entry_over_copy=round(med(ts["entry"]) / med(ts["copy"]), 2),
                   torch_over_kernel=round(med(ts["torch"]) / med(ts["kernel"]), 1), counts_equal_torch=same,
                   n_both=float(got[0, 2]), brier=round(float(got[0, 4] / got[0, 2]), 4))
        score_rows.append(row)
        report("occ_score", med(ts["entry"]), nbytes, **row)
    out = os.environ.get("VIDAR_KBENCH_OUT")
    path = Path(out) if out else ROOT / "profiles" / "kbench_occ_score.md"
    path.write_text(
        "# Occupancy score on an MI355X: `python tools/kbench.py occ_score`\n\n"
        f"Volume {Z} x {Y} x {X}, step 1, the {p.shape[0]} rays of `vidar_amd.forecast.lidar_pattern()` from the volume's centre,\n"
        "end points 4 - 120 voxels out (seeded).  `sweep_evidence` (`vidar_sweep_evidence_f32`, no volume read) next to\n"
        "`ray_occupancy` (`vidar_ray_occupancy_f32`, random-normal logits) on the same rays, in the same process, the two ops\n"
        "alternating; `default` adds with fp32 atomics into 8 private copies of both volumes, `deterministic` measures and\n"
        "then adds in 64-bit fixed point.  `waypoints with a weight`: the waypoints sweep_evidence marches with a_k > 0\n"
        "(ray_occupancy scatters every live waypoint of all K).  Then `occupancy_score` (`vidar_occ_score_f32`, 2 thresholds,\n"
        "10 bins) on the K = 512 grids for 1 and 7 segments, next to a torch program on the device that builds the same table\n"
        "(`tools/kbench.py _occ_table_torch`) and to a device-to-device copy of the same 16 B per voxel (which also WRITES\n"
        "16 B per voxel).  `entry`: `vidar_occ_score_f32` called on a table and a workspace allocated once -- the two launches\n"
        "without the wrapper's allocations.  HIP events, 3 repeats of 2 warm-up + 20 timed calls; spread = (max - min) / median.  Each call\n"
        "allocates its outputs and its workspace.\n\n"
        "```\n" + json.dumps({"device": torch.cuda.get_device_name(0)}) + "\n"
        + "\n".join(json.dumps(dict(op="sweep_evidence", **r)) for r in rows) + "\n"
        + "\n".join(json.dumps(dict(op="occ_score", **r)) for r in score_rows) + "\n```\n\n"
        "| R | K | mode | sweep_evidence ms (median) | spread | ray_occupancy ms (median) | spread | sweep / occupancy | waypoints with a weight |\n"
        "|---|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['R']} | {r['K']} | {r['mode']} | {r['sweep_evidence_median_ms']} | {r['sweep_evidence_spread']} | "
                  f"{r['ray_occupancy_median_ms']} | {r['ray_occupancy_spread']} | {r['ratio']} | "
                  f"{r['waypoints_with_a_weight']} |\n" for r in rows)
        + "\n| segments | voxels each | read MB | occupancy_score ms (median) | spread | entry ms (median) | spread | entry GB/s read | copy ms | occupancy_score / copy | entry / copy | torch ms | torch / occupancy_score | counts equal torch's |\n"
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['S']} | {r['V']} | {r['read_MB']} | {r['kernel_median_ms']} | {r['kernel_spread']} | {r['entry_median_ms']} | "
                  f"{r['entry_spread']} | {r['entry_GBps']} | {r['copy_median_ms']} | {r['kernel_over_copy']} | "
                  f"{r['entry_over_copy']} | {r['torch_median_ms']} | {r['torch_over_kernel']} | "
                  f"{r['counts_equal_torch']} |\n" for r in score_rows))


def bench_voxel_occupancy(which):
    """the dense occupancy query (vidar_voxel_occupancy_f32: one ray per voxel) on a 16 x 200 x 200 volume, step 1, at
    K = 512 (register form) and K = 1026 (streamed), one frame and seven.  In the same process, the ops alternating:
      * ray_stats and point_occupancy on the same 640 000 rays per frame materialised as listed end points -- the same two
        visits of every waypoint, plus 12 bytes of end point read and 16 (ray_stats) / 8 bytes stored per ray;
      * what users run today, one frame: ray_occupancy on the 34 560 rays of vidar_amd.forecast.lidar_pattern() and
        ray_occupancy_cam on 6 cameras of 900 x 1600 pixels at strides 8 and 4 (default mode: fp32 atomics),
    and under every source the count of voxels whose evidence hit + free reaches 0.5 (the two evidences have different
    units: a probability for the dense form, waypoints for the splat).  HIP events, three repeats of 2 warm-up + 5 timed
    calls; the spread is (max - min) / median over the repeats.  Writes profiles/kbench_voxel_occupancy.md."""
    from vidar_amd import forecast as FC
    from vidar_amd.plugin.dense_heads.ray_ops import (point_occupancy, ray_occupancy, ray_occupancy_cam, ray_stats,
                                                      voxel_occupancy)
    from vidar_amd.synthetic import PC_RANGE, camera_matrices
    dev = torch.device("cuda", 0)
    Z, Y, X, C, H, W = 16, 200, 200, 6, 900, 1600
    med = lambda v: float(np.median(v))
    spread = lambda v: (max(v) - min(v)) / med(v)
    seen = lambda hit, free: int((hit + free >= 0.5).sum())
    touched = lambda hit, free: int((hit + free > 0).sum())
    rows, splat_rows = [], []

    def times(fns, it=5):
        ts = {name: [] for name in fns}
        for _ in range(3):
            for name, fn in fns.items():
                ts[name].append(timeit(fn, warm=2, it=it))
        return ts

    for F_ in (1, 7):
        sigma = torch.randn(F_, Z, Y, X, generator=torch.Generator().manual_seed(0)).to(dev)
        o = torch.tensor([[X / 2.0, Y / 2.0, Z / 4.0]], device=dev).repeat(F_, 1)
        z, y, x = torch.meshgrid(torch.arange(Z, device=dev), torch.arange(Y, device=dev), torch.arange(X, device=dev),
                                 indexing="ij")
        p = (torch.stack([x, y, z], -1).reshape(-1, 3).float() + 0.5).repeat(F_, 1)
        ti = torch.arange(F_, device=dev).repeat_interleave(Z * Y * X).float()
        for K in (512, 1026):
            hit, free = voxel_occupancy(sigma, o, 1.0, K)
            listed = point_occupancy(sigma, o, p, ti, 1.0, K)
            same = bool(torch.equal(torch.stack([hit.reshape(-1), free.reshape(-1)], 1), listed))
            ts = times({"voxel_occupancy": lambda: voxel_occupancy(sigma, o, 1.0, K),
                        "ray_stats": lambda: ray_stats(sigma, o, p, ti, 1.0, K),
                        "point_occupancy": lambda: point_occupancy(sigma, o, p, ti, 1.0, K)})
            t, ts_stats = med(ts["voxel_occupancy"]), med(ts["ray_stats"])
            row = dict(F=F_, R=p.shape[0], K=K, form="register" if K == 512 else "streamed",
                       voxel_occupancy_ms=[round(v, 3) for v in ts["voxel_occupancy"]], voxel_occupancy_median_ms=round(t, 3),
                       voxel_occupancy_spread=round(spread(ts["voxel_occupancy"]), 4),
                       ray_stats_median_ms=round(ts_stats, 3), ray_stats_spread=round(spread(ts["ray_stats"]), 4),
                       point_occupancy_median_ms=round(med(ts["point_occupancy"]), 3),
                       point_occupancy_spread=round(spread(ts["point_occupancy"]), 4),
                       dense_over_ray_stats=round(t / ts_stats, 4), equals_point_form=same,
                       voxels=hit.numel(), voxels_seen=seen(hit, free), voxels_touched=touched(hit, free), ns_per_ray=round(t * 1e6 / p.shape[0], 2))
            rows.append(row)
            report("voxel_occupancy", t, **row)
        del p, ti

    sigma = torch.randn(1, Z, Y, X, generator=torch.Generator().manual_seed(0)).to(dev)
    o = torch.tensor([[X / 2.0, Y / 2.0, Z / 4.0]], device=dev)
    sweep = o + FC.lidar_pattern().to(dev)
    ti = torch.zeros(sweep.shape[0], device=dev)
    m = FC.pix2vox(camera_matrices(img_hw=(H, W))[:C], PC_RANGE, Y, X, Z).to(dev)
    for K in (512, 1026):
        dense = next(r for r in rows if r["F"] == 1 and r["K"] == K)
        sources = [("sweep", "-", sweep.shape[0], lambda: ray_occupancy(sigma, o, sweep, ti, 1.0, K))]
        for stride in (8, 4):
            Hs, Ws = -(-H // stride), -(-W // stride)
            geom = ((Hs, Ws), stride / 2.0, stride / 2.0, float(stride), float(stride))
            sources.append(("camera", stride, C * Hs * Ws, lambda geom=geom: ray_occupancy_cam(sigma, m, *geom, 1.0, K)))
        for name, stride, R, fn in sources:
            hit, free = fn()
            ts = times({"splat": fn})["splat"]
            row = dict(rays=name, stride=stride, R=R, K=K, splat_ms=[round(v, 3) for v in ts], splat_median_ms=round(med(ts), 3),
                       splat_spread=round(spread(ts), 4), voxels_seen=seen(hit, free), voxels_touched=touched(hit, free),
                       seen_per_ms=round(seen(hit, free) / med(ts)), dense_median_ms=dense["voxel_occupancy_median_ms"],
                       dense_voxels_seen=dense["voxels_seen"], dense_voxels_touched=dense["voxels_touched"],
                       dense_seen_per_ms=round(dense["voxels_seen"] / dense["voxel_occupancy_median_ms"]))
            splat_rows.append(row)
            report("voxel_occupancy_vs_splat", med(ts), **row)
    out = os.environ.get("VIDAR_KBENCH_OUT")
    path = Path(out) if out else ROOT / "profiles" / "kbench_voxel_occupancy.md"
    path.write_text(
        "# The dense occupancy query on an MI355X: `python tools/kbench.py voxel_occupancy`\n\n"
        f"Volume F x {Z} x {Y} x {X}, random-normal logits (seed 0), step 1, every origin at the volume's centre, extent 1.\n"
        "`voxel_occupancy` (`vidar_voxel_occupancy_f32`) marches one ray per voxel and never stores the rays; `ray_stats`\n"
        "(`vidar_ray_stats_f32`) and `point_occupancy` (`vidar_point_occupancy_f32`) march the same rays materialised as listed\n"
        "end points.  K = 512 runs the register form, K = 1026 the streamed one.  HIP events, the ops alternating, 3 repeats\n"
        "of 2 warm-up + 5 timed calls; spread = (max - min) / median.  Each call allocates its outputs.  `seen` = voxels with\n"
        "hit + free >= 0.5, `touched` = voxels with hit + free > 0 (an answer at a floor of 0).\n\n"
        "```\n" + json.dumps({"device": torch.cuda.get_device_name(0)}) + "\n"
        + "\n".join(json.dumps(dict(op="voxel_occupancy", **r)) for r in rows) + "\n"
        + "\n".join(json.dumps(dict(op="voxel_occupancy_vs_splat", **r)) for r in splat_rows) + "\n```\n\n"
        "| F | R | K | voxel_occupancy ms (median) | spread | ray_stats ms | spread | point_occupancy ms | spread | dense / ray_stats | "
        "equals the point form | seen | touched |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['F']} | {r['R']} | {r['K']} | {r['voxel_occupancy_median_ms']} | {r['voxel_occupancy_spread']} | "
                  f"{r['ray_stats_median_ms']} | {r['ray_stats_spread']} | {r['point_occupancy_median_ms']} | "
                  f"{r['point_occupancy_spread']} | {r['dense_over_ray_stats']} | {r['equals_point_form']} | "
                  f"{r['voxels_seen']} of {r['voxels']} | {r['voxels_touched']} |\n" for r in rows)
        + "\nWhat users run today, one frame, default mode (`ray_occupancy` on the rays of `vidar_amd.forecast.lidar_pattern()`,\n"
        f"`ray_occupancy_cam` on {C} cameras of {H} x {W} pixels), next to the dense form at the same K.  The evidence units\n"
        "differ -- waypoints of the rays that happened to pass for the splat, the probability the voxel's own ray still has for\n"
        "the dense form -- so `seen` compares answers given, not their quality.\n\n"
        "| rays | stride | R | K | splat ms (median) | spread | touched | seen | seen / ms | dense ms | dense touched | dense seen | "
        "dense seen / ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n"
        + "".join(f"| {r['rays']} | {r['stride']} | {r['R']} | {r['K']} | {r['splat_median_ms']} | {r['splat_spread']} | "
                  f"{r['voxels_touched']} | {r['voxels_seen']} | {r['seen_per_ms']} | {r['dense_median_ms']} | "
                  f"{r['dense_voxels_touched']} | {r['dense_voxels_seen']} | "
                  f"{r['dense_seen_per_ms']} |\n" for r in splat_rows))


if __name__ == "__main__":
    import os
    if os.environ.get("VIDAR_MSDA_ITEM_ORDER") is not None:         # A/B of the gather kernels' item order (0 banded, 1 head-major)
        from vidar_amd._lib import lib
        lib().vidar_msda_set_item_order(int(os.environ["VIDAR_MSDA_ITEM_ORDER"]))
    if os.environ.get("VIDAR_GEMM_VARIANT") is not None:               # A/B of the GEMM kernel's structure (0 classic, 1 / 2 wave-specialised)
        from vidar_amd._lib import lib
        lib().vidar_gemm_set_variant(int(os.environ["VIDAR_GEMM_VARIANT"]))
    which = sys.argv[1:] or ["dvr", "knn", "msda", "lr", "ray"]
    print(json.dumps({"device": torch.cuda.get_device_name(0)}))
    for w in which:
        globals()["bench_" + w](w)
