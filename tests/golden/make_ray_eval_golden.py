"""Golden values for the device ray-error metric (csrc/ray_eval_math.h, csrc/ray_eval.hip) from the REFERENCE's
utils/eval_utils.py, executed in place; `chamferdist` is stubbed by an fp64 brute-force nearest neighbour (lowest index
on ties -- the reference hands fp64 spherical coordinates to a kernel templated on the scalar type):
    python tests/golden/make_ray_eval_golden.py
writes tests/golden/ray_eval_cases.npz.  Inputs are fp32-valued (stored as float32, widened for the reference).

Cases (`names` lists them):
  on_rays_<i>   origin i, the predictions sit on the ground-truth rays at another depth (the pipeline's shape, P == G);
                G = 255, 256, 257, 539, 1
  indep_<j>     origin j % 5, independent clouds; P = 1, 63, 64, 65, C, C + 1, 2 C + 3 (C = 1024, the kernel's LDS chunk)
                against G = 539, 257, 256, 255, 539, 257, 256.  The four small P have fewer predictions than rays; the
                three sizes around the chunk cannot (no G is that large).
  tie           origin 0, predictions p and 2 p (exact in fp32) of the same direction: the lower index must win
Every case with more than one ray carries the hand-placed rays of `hand_rays`: axis-parallel ones, ends in the 0.02 m
shell around the box, one shorter than 1 cm, one that leads away from the box (it misses the volume when the origin is
outside).

Per case <n>: <n>_pred [P,3] f32, <n>_gt [G,3] f32, <n>_origin [3] f32; <n>_l1, <n>_absrel (compute_ray_errors);
<n>_clamp_o / <n>_clamp_p [G,3] f64 and <n>_invalid [G] bool (clamp(gt, origin, return_invalid_mask=True));
<n>_interp [count,3] f64 (return_interpolated_pcd=True, one row per COUNTED ray, in order); <n>_nn [G] i32: the row of
<n>_pred the stub chose, -1 for an uncounted ray; <n>_terms [G,2] f64: the (L1, AbsRel) term of every ray from the
reference's clamp of <n>_interp, 0 where the ray contributes nothing (their sums over the count are <n>_l1 / <n>_absrel)."""
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(Path(__file__).parent))
import ref_import  # noqa: E402

CHUNK = 1024          # kChunk of csrc/ray_eval.hip
ORIGINS = [(1.0, -2.0, 0.3), (80.0, 5.0, 1.0), (0.5, 0.25, 6.0), (-75.0, -72.0, -6.0), (69.99, 0.0, 4.51)]
MIN_GAP = 1e-12       # best against second-best squared angular distance of every counted ray
last = {}             # what the stub saw in the latest call


class Fp64Chamfer(torch.nn.Module):
    def forward(self, src, tgt, bidirectional=False, reverse=False, reduction="mean"):
        assert reverse and not bidirectional and src.dtype == torch.float64 and tgt.dtype == torch.float64
        p, g = src[0].numpy(), tgt[0].numpy()
        d = np.zeros((g.shape[0], p.shape[0]))
        for k in range(3):                                # dist += diff * diff, coordinate by coordinate
            diff = g[:, None, k] - p[None, :, k]
            d = d + diff * diff
        idx = d.argmin(1)                                 # the first of equal minima: the lowest index
        best = d[np.arange(len(g)), idx]
        if p.shape[0] > 1:
            d[np.arange(len(g)), idx] = np.inf
            last["gap"] = float((d.min(1) - best).min()) if len(g) else np.inf
        else:
            last["gap"] = np.inf
        last["idx"] = idx
        return torch.from_numpy(best).sum(), (torch.from_numpy(best)[None], torch.from_numpy(idx)[None])


sys.modules["chamferdist"] = types.SimpleNamespace(ChamferDistance=Fp64Chamfer)
ref = ref_import.load_file("ref_eval_utils_f64", ref_import.PLUGIN / "bevformer/utils/eval_utils.py")


def hand_rays(o):
    o = np.asarray(o, np.float64)
    away = np.where(o >= 0, 1.0, -1.0) * [30.0, 30.0, 3.0]
    return np.array([
        o + [25, 0, 0], o + [-200, 0, 0], o + [0, -30, 0], o + [0, 200, 0], o + [0, 0, 2],      # axis-parallel
        [70.01, 3.0, 1.0], [-5.0, -70.015, 0.5], [2.0, 3.0, 4.51],                              # end in the 0.02 shell
        o + [0.003, 0.004, 0.0],                                                                # shorter than 1 cm
        o + away,                                                                               # leads away from the box
    ])


def cloud(rng, n):
    near = rng.uniform(-60, 60, (n, 3)) * [1, 1, 0.05]
    far = rng.uniform(-120, 120, (n, 3)) * [1, 1, 0.08]
    return np.where(rng.uniform(size=(n, 1)) < 0.8, near, far)


def gt_cloud(rng, o, n):
    if n == 1:
        return np.array([[12.5, -30.25, 0.75]], np.float32)
    hand = hand_rays(o)
    return np.concatenate([cloud(rng, n - len(hand)), hand]).astype(np.float32)


def run(name, pred, gt, origin, out, tie=False):
    pred, gt, origin = (np.ascontiguousarray(a, np.float32) for a in (pred, gt, origin))
    p64, g64, o64 = pred.astype(np.float64), gt.astype(np.float64), origin.astype(np.float64)
    dev = torch.device("cpu")
    l1, absrel = ref.compute_ray_errors(p64.copy(), g64.copy(), o64.copy(), dev)       # must not raise
    idx, gap = last["idx"], last["gap"]
    interp = ref.compute_ray_errors(p64.copy(), g64.copy(), o64.copy(), dev, return_interpolated_pcd=True)
    co, cp, inv = ref.clamp(g64.copy(), o64.copy(), return_invalid_mask=True)
    kept = np.flatnonzero(np.sqrt(((p64 - o64) ** 2).sum(1)) > 1e-2)
    counted = np.sqrt(((g64 - o64) ** 2).sum(1)) > 1e-2
    nn = np.full(len(gt), -1, np.int32)
    nn[counted] = kept[idx]
    assert interp.shape == (int(counted.sum()), 3)
    if not tie:
        assert gap >= MIN_GAP, (name, gap)
    # rays that contribute nothing: invalid after clamping, or shorter than 0.01 after clamping, or uncounted
    dc = np.sqrt(((cp - co) ** 2).sum(1))
    lost = inv | ~(np.where(inv, 1.0, dc) > 0.01) | ~counted
    assert lost.mean() <= 0.25, (name, lost.mean())
    _, ip, _ = ref.clamp(interp.copy(), o64.copy(), return_invalid_mask=True)
    rows = np.flatnonzero(counted)
    ok = ~lost[rows]
    e = np.sqrt(((cp[rows] - ip) ** 2).sum(1))
    terms = np.zeros((len(gt), 2))
    terms[rows[ok]] = np.stack([e[ok], e[ok] / dc[rows][ok]], 1)
    np.testing.assert_allclose(terms.sum(0) / counted.sum(), [l1, absrel], rtol=1e-12)
    out[f"{name}_terms"] = terms
    out.update({f"{name}_pred": pred, f"{name}_gt": gt, f"{name}_origin": origin, f"{name}_l1": l1, f"{name}_absrel": absrel,
                f"{name}_clamp_o": co, f"{name}_clamp_p": cp, f"{name}_invalid": inv, f"{name}_interp": interp,
                f"{name}_nn": nn})
    print(f"{name:10s} P {len(pred):5d} G {len(gt):4d} counted {int(counted.sum()):4d} invalid {int(inv.sum()):3d} "
          f"lost {lost.mean():.3f} gap {gap:.3e} l1 {l1:.6f} absrel {absrel:.6f}")


def main():
    rng = np.random.default_rng(20)
    out, names = {}, []
    for i, (o, G) in enumerate(zip(ORIGINS, (255, 256, 257, 539, 1))):
        o32 = np.asarray(o, np.float32)
        gt = gt_cloud(rng, o32, G)
        pred = o32.astype(np.float64) + (gt.astype(np.float64) - o32) * rng.uniform(0.6, 1.4, (G, 1))
        names.append(f"on_rays_{i}")
        run(names[-1], pred, gt, o32, out)
    for j, (P, G) in enumerate(zip((1, 63, 64, 65, CHUNK, CHUNK + 1, 2 * CHUNK + 3), (539, 257, 256, 255, 539, 257, 256))):
        o32 = np.asarray(ORIGINS[j % 5], np.float32)
        names.append(f"indep_{j}")
        run(names[-1], cloud(rng, P), gt_cloud(rng, o32, G), o32, out)
    # the tie: p and 2 p have the same direction exactly; ray 0 finds (2 p, p) at rows (0, 1), ray 1 (p, 2 p) at (2, 3)
    g = np.array([[3.0, 4.0, 0.5], [-6.0, 2.5, -0.25], [1.0, -8.0, 1.0]], np.float32)
    pred = np.array([2 * g[0], g[0], g[1], 2 * g[1], 0.5 * g[2]], np.float32) * np.float32(0.75)
    names.append("tie")
    run("tie", pred, g * np.float32(1.5), np.zeros(3, np.float32), out, tie=True)
    assert out["tie_nn"].tolist() == [0, 2, 4], out["tie_nn"]
    out["names"] = np.array(names)
    np.savez_compressed(Path(__file__).parent / "ray_eval_cases.npz", **out)


if __name__ == "__main__":
    main()
