"""CPU: libvidar_hip.so builds for gfx950, loads, and exports every symbol include/vidar_hip.h
declares (no compute calls without a GPU); the product fails loudly without its library/GPU."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def declared_symbols():
    text = (ROOT / "include" / "vidar_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vidar_\w+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    from vidar_amd import build
    lib_path = build.build(verbose=False)
    lib = ctypes.CDLL(str(lib_path))
    names = declared_symbols()
    assert len(names) >= 28
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in vidar_hip.h but not exported: {missing}"
    assert lib.vidar_abi_version() >= 1
    assert lib.vidar_dvr_max_d() == 1446 and lib.vidar_dvxlr_max_d() == 1026


# the 14 parameter types the header uses -> the kind code of vidar_amd._lib._ABI ("name[6]" parameters count as pointers)
SCALAR_KINDS = {"int": "i", "float": "f", "int64_t": "l", "size_t": "z", "uint32_t": "u"}
POINTEES = {"void", "float", "int64_t", "int32_t", "uint8_t"}


def header_prototypes():
    """name -> (return kind, [parameter kinds]) of every prototype of include/vidar_hip.h"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vidar_hip.h").read_text(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(\w+)\s+(vidar_\w+)\s*\(([^()]*)\)\s*;", text):
        kinds = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(const\s+)?(\w+)\s*(\*?)\s*\w+\s*(\[\d*\])?\s*", prm)
            assert m, f"{name}: cannot read the parameter {prm!r}"
            const, base, star, array = m.groups()
            if star or array:
                assert base in POINTEES, f"{name}: unknown pointer type in {prm!r}"
                kinds.append("p")
            else:
                assert base in SCALAR_KINDS and not const, f"{name}: unknown parameter type in {prm!r}"
                kinds.append(SCALAR_KINDS[base])
        assert ret in ("int", "size_t"), f"{name}: unknown return type {ret!r}"
        assert name not in out, f"{name} is declared twice"
        out[name] = (SCALAR_KINDS[ret], kinds)
    return out


def test_prototype_table_equals_the_header():
    from vidar_amd import _lib
    protos = header_prototypes()
    assert len(protos) == len(declared_symbols()), sorted(set(declared_symbols()) - set(protos))
    assert sorted(_lib._ABI) == sorted(protos)
    for name, (ret, kinds) in protos.items():
        restype, argtypes = _lib.signature(name)
        assert restype is _lib._KIND[ret], name
        assert len(argtypes) == len(kinds), name
        assert argtypes == [_lib._KIND[k] for k in kinds], name
    assert (_lib._KIND["p"], _lib._KIND["i"], _lib._KIND["l"]) == (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64)
    assert (_lib._KIND["z"], _lib._KIND["f"], _lib._KIND["u"]) == (ctypes.c_size_t, ctypes.c_float, ctypes.c_uint32)


def test_prototype_table_is_applied_on_load():
    from vidar_amd._lib import lib
    L = lib()
    protos = header_prototypes()
    for name, (ret, kinds) in protos.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(kinds), name
        assert (fn.restype is ctypes.c_size_t) == (ret == "z"), name
        assert fn.restype is (ctypes.c_size_t if ret == "z" else ctypes.c_int), name
    assert sum(ret == "z" for ret, _ in protos.values()) == 12


def test_declare_names_a_symbol_the_library_lacks():
    from vidar_amd._lib import VidarHipError, declare
    with pytest.raises(VidarHipError, match="vidar_abi_version"):
        declare(ctypes.CDLL(None))          # the process itself: exports none of the entries


def test_64_bit_values_cross_the_boundary():
    """host-only arithmetic, linear in `rows`: an int64_t argument cut to 32 bits would arrive as 0 and give 0 bytes,
    a size_t result read as int would wrap"""
    from vidar_amd._lib import lib
    f = lib().vidar_drop_add_ln_bwd_workspace_bytes
    a, b = f(1 << 39), f(1 << 40)
    assert a > 1 << 32 and b > 1 << 32
    assert b > a


def test_wrong_argument_types_fail_in_python():
    """1.5 for the `int N` of vidar_dvr_init_f32 never reaches C.  The correctly typed null call that returns 0 with no
    GPU is made on vidar_dvr_render_forward_f32: it answers M == 0 before any HIP call, while dvr_init clears its output
    first (hipMemsetAsync: hipErrorNoDevice on a machine without a GPU)."""
    from vidar_amd._lib import lib
    L = lib()
    with pytest.raises(ctypes.ArgumentError):
        L.vidar_dvr_init_f32(None, None, None, 1.5, 0, 1, 1, 1, 1, None)
    assert L.vidar_dvr_render_forward_f32(None, None, None, None, None, None, 1, 0, 1, 1, 1, 1, 1, 0, None) == 0
    with pytest.raises(ctypes.ArgumentError):
        L.vidar_dvr_render_forward_f32(None, None, None, None, None, None, 1.5, 0, 1, 1, 1, 1, 1, 0, None)


def test_no_cpu_fallback():
    """CPU tensors are rejected (CHECK_CUDA semantics), nothing silently runs on the host."""
    from vidar_amd.third_lib import dvxlr
    from vidar_amd.third_lib.chamferdist import knn_points
    from vidar_amd.plugin.modules.multi_scale_deformable_attn_function import multi_scale_deformable_attn
    with pytest.raises(RuntimeError):
        dvxlr.render(torch.zeros(1, 1, 2, 2, 2), torch.zeros(1, 1, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4))
    with pytest.raises(RuntimeError):
        knn_points(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    with pytest.raises(RuntimeError):
        multi_scale_deformable_attn(torch.zeros(1, 4, 8, 32), torch.tensor([[2, 2]]), torch.tensor([0]),
                                    torch.zeros(1, 3, 8, 1, 4, 2), torch.zeros(1, 3, 8, 1, 4))


def test_product_never_imports_oracle():
    for f in (ROOT / "vidar_amd").rglob("*.py"):
        src = f.read_text()
        assert "import oracle" not in src and "from oracle" not in src, f
    for f in (ROOT / "vidar_amd" / "csrc").glob("*"):
        if f.is_file() and f.suffix in (".hip", ".h"):
            assert "oracle" not in f.read_text().lower(), f
    # tools/ (benchmarks, profiling helpers) must not lean on the checker either, directly or through tests/
    for f in (ROOT / "tools").rglob("*.py"):
        src = f.read_text()
        assert "import oracle" not in src and "from oracle" not in src, f
        assert "from test_" not in src and "import test_" not in src, f
    # bench.py: only the two functions of the cpu_baseline leg (run in a child process, outside the timed region)
    lines = (ROOT / "bench.py").read_text().splitlines()
    uses = [i for i, l in enumerate(lines) if "from oracle" in l or "import oracle" in l]

    def span(name):
        start = next(i for i, l in enumerate(lines) if l.startswith(f"def {name}("))
        return start, next(i for i, l in enumerate(lines) if i > start and l.startswith("def "))
    spans = [span("cpu_baseline"), span("cpu_baseline_ops")]
    assert uses and all(any(a < i < b for a, b in spans) for i in uses), uses
