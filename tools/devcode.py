"""Device-code tools that need no GPU.

    python tools/devcode.py diff A.hip B.hip [-- extra hipcc flags]    # is the gfx950 code of two sources identical?
    python tools/devcode.py head-diff vidar_amd/csrc/dcn.hip [-- flags] # working tree vs the committed file (HEAD)
    python tools/devcode.py asm vidar_amd/csrc/dcn.hip KERNEL [-- flags] # disassembly of the kernels whose name contains KERNEL
    python tools/devcode.py lib-diff PARENT.so TREE.so ['old<*>=new<*, T>' ...]  # two built libraries, kernel by kernel

lib-diff is for changes that touch headers (head-diff compiles HEAD's source against the working tree's headers): build
the parent commit elsewhere and compare the libraries.  Kernels are matched by their short demangled name; an
`old=new` pair maps a renamed kernel, `*` standing for the same text on both sides.

Used to prove that a refactor, or a compile-time variant that is off by default, leaves the shipped device code
untouched (the round's rule: nothing that changes device code goes in without a GPU run), and to read what the
compiler made of a loop (loads in flight, s_waitcnt placement).  Per-file flags are those of vidar_amd/build.py."""
import difflib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from kernel_resources import LLVM, code_objects, demangle, short  # noqa: E402
from vidar_amd.build import COMMON, HIPCC, PER_FILE  # noqa: E402


def disasm(src, extra, work, name=None):
    src = Path(src)
    so = work / f"{src.stem}_{abs(hash((str(src), tuple(extra))))}.so"
    flags = COMMON + PER_FILE.get(name or src.name, []) + list(extra)
    subprocess.run([HIPCC, *flags, "-shared", str(src), "-o", str(so)], check=True)
    sub = work / (so.stem + "_co")
    sub.mkdir()
    text = []
    for co in code_objects(so, sub):
        out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(co)], text=True, capture_output=True, check=True).stdout
        text += [ln for ln in out.splitlines() if "file format" not in ln]
    return text


def kernels(text):
    cur, body = None, {}
    for ln in text:
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur and ln.strip():
            body[cur].append(re.sub(r"\s*//.*", "", ln).strip())
    return body


def lib_kernels(so, work):
    """{short demangled name: instructions} of a built library; a name that several translation units carry (the
    shells' own kernels) gets ' #2', ' #3' in the order of the code objects"""
    work.mkdir()
    body = {}
    for co in code_objects(Path(so), work):
        out = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(co)], text=True, capture_output=True, check=True).stdout
        ks = kernels(out.splitlines())
        for mangled, name in zip(ks, map(short, demangle(list(ks)))):
            n, key = 1, name
            while key in body:
                n += 1
                key = f"{name} #{n}"
            body[key] = ks[mangled]
    return body


def rename(name, pairs):
    """`name` under the first 'old=new' pair whose old side matches it ('*': any text, repeated in `new`), else itself"""
    for pair in pairs:
        old, new = pair.split("=", 1)
        m = re.fullmatch("(.*)".join(map(re.escape, old.split("*"))) + r"( #\d+)?", name)
        if m:
            *stars, dup = m.groups()
            parts = new.split("*")             # the i-th `*` of `new` is the i-th of `old`
            return "".join(a + b for a, b in zip(parts, stars[:len(parts) - 1] + [""])) + (dup or "")
    return name


def lib_diff(parent, tree, pairs, work):
    ka = {rename(k, pairs): (k, v) for k, v in lib_kernels(parent, work / "a").items()}
    kb = lib_kernels(tree, work / "b")
    same = 0
    for k in sorted(set(ka) | set(kb)):
        (old, a), b = ka.get(k, (k, None)), kb.get(k)
        if a == b:
            same += 1
            continue
        was = "" if old == k else f"  (was {old})"
        if a is None or b is None:
            print(f"only in {'tree' if a is None else 'parent'}: {k}")
        else:
            print(f"differs: {k}{was}  ({len(a)} -> {len(b)} instructions)")
            for ln in difflib.unified_diff(a, b, "parent", "tree", n=0, lineterm=""):
                if not ln.startswith(("---", "+++", "@@")):
                    print("    " + ln)
    print(f"identical: {same} of {len(set(ka) | set(kb))} kernels")
    return 0 if same == len(set(ka) | set(kb)) else 1


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        i = argv.index("--")
        argv, extra = argv[:i], argv[i + 1:]
    cmd = argv[0]
    with tempfile.TemporaryDirectory() as d:
        work = Path(d)
        if cmd in ("diff", "head-diff"):
            if cmd == "diff":
                a, b, name = Path(argv[1]), Path(argv[2]), Path(argv[2]).name
            else:
                b = Path(argv[1]).resolve()
                name = b.name
                a = work / ("HEAD_" + name)
                a.write_bytes(subprocess.run(["git", "-C", str(ROOT), "show", f"HEAD:{b.relative_to(ROOT)}"],
                                             capture_output=True, check=True).stdout)
            ka, kb = kernels(disasm(a, extra, work, name)), kernels(disasm(b, extra, work, name))
            changed = [k for k in sorted(set(ka) | set(kb)) if ka.get(k) != kb.get(k)]
            if not changed:
                print(f"identical device code: {len(kb)} kernels")
                return 0
            for k in changed:
                print(f"differs: {k[:100]}  ({len(ka.get(k, []))} -> {len(kb.get(k, []))} instructions)")
            return 1
        if cmd == "lib-diff":
            return lib_diff(argv[1], argv[2], argv[3:], work)
        if cmd == "asm":
            for k, body in kernels(disasm(argv[1], extra, work)).items():
                if argv[2] in k:
                    print(f"== {k}  ({len(body)} instructions)")
                    for n, ln in enumerate(body):
                        print(f"{n:5d}  {ln}")
            return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
