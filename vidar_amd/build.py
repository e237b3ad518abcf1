"""Build libvidar_hip.so (the C-ABI shared library) with hipcc for gfx950.

In-tree build: objects under vidar_amd/csrc/_obj/, library at vidar_amd/libvidar_hip.so
(git-ignored, but shipped to the GPU box by gpurun).  hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
OBJ = CSRC / "_obj"
LIB = PKG / "libvidar_hip.so"

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# -ffp-contract=off: ray/voxel traversal decisions and KNN distances must follow the reference's
# IEEE operation order exactly (bit-exact index lists); per-file flags can relax this.
COMMON = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
    "-munsafe-fp-atomics", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-Wall", "-Wno-unused-function",
]
PER_FILE: dict[str, list[str]] = {
    # pure fp32 interpolation arithmetic, tolerance-checked: let the compiler fuse multiply-adds
    "msda.hip": ["-ffp-contract=fast"],
    "dcn.hip": ["-ffp-contract=fast"],
    "affine_act.hip": ["-ffp-contract=fast"],
    "norm_fuse.hip": ["-ffp-contract=fast"],
    # the image pipeline must reproduce numpy's fp32 results bit for bit (a uint8 cast follows): every operation rounds
    # on its own, whatever COMMON says tomorrow
    "img_prep.hip": ["-ffp-contract=off"],
    # the same for the fp64 ray errors against the reference's numpy (csrc/ray_eval_math.h)
    "ray_eval.hip": ["-ffp-contract=off"],
    # and for the fp64 duals of the assignment: the host program of the tests must take the same decisions
    # (csrc/det_assign_math.h)
    "det_assign.hip": ["-ffp-contract=off"],
    # and for the fp32 decisions of the occupancy score: a voxel on a floor or a threshold must fall on the side the
    # torch restatement and the host program put it (csrc/occ_score_math.h)
    "occ_score.hip": ["-ffp-contract=off"],
}


def sources() -> list[Path]:
    return sorted(CSRC.glob("*.hip"))


def _stamp(src: Path, flags: list[str]) -> str:
    h = hashlib.sha256()
    h.update(src.read_bytes())
    for hdr in sorted(list(CSRC.glob("*.h")) + list((ROOT / "include").glob("*.h"))):
        h.update(hdr.read_bytes())
    h.update(" ".join(flags).encode())
    return h.hexdigest()


def _compile(src: Path, verbose: bool) -> Path:
    # VIDAR_EXTRA_HIPCC_FLAGS: extra flags (the -D switches of the tuning sweeps / staged variants) for every source,
    # or only for the sources named in VIDAR_EXTRA_HIPCC_ONLY (comma separated file names) -- the others keep their
    # objects, so a one-file variant rebuilds in seconds
    only = [n for n in os.environ.get("VIDAR_EXTRA_HIPCC_ONLY", "").split(",") if n]
    extra = os.environ.get("VIDAR_EXTRA_HIPCC_FLAGS", "").split() if (not only or src.name in only) else []
    flags = COMMON + PER_FILE.get(src.name, []) + extra
    obj = OBJ / (src.stem + ".o")
    stamp = OBJ / (src.stem + ".stamp")
    want = _stamp(src, flags)
    if obj.exists() and stamp.exists() and stamp.read_text() == want:
        return obj
    cmd = [HIPCC, *flags, "-c", str(src), "-o", str(obj)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    stamp.write_text(want)
    return obj


def build(verbose: bool = True, force: bool = False) -> Path:
    OBJ.mkdir(parents=True, exist_ok=True)
    if force:
        for f in OBJ.glob("*.stamp"):
            f.unlink()
    srcs = sources()
    if not srcs:
        raise RuntimeError("no HIP sources found")
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(lambda s: _compile(s, verbose), srcs))
    newest = max(o.stat().st_mtime for o in objs)
    if force or not LIB.exists() or LIB.stat().st_mtime < newest:
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *map(str, objs), "-o", str(LIB)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(verbose=True, force="--force" in sys.argv)
    print(LIB)
