#!/usr/bin/env python3
"""One line per gfx950 kernel of csrc/*.hip: resources and a hash of the instruction text (no GPU needed).

    python tools/kernel_manifest.py [--root DIR] [file.hip ...] > manifest.txt
    python tools/kernel_manifest.py --diff before.txt after.txt ['regex=replacement' ...]

hipcc with the flags of ffwm_amd/build.py plus ``--offload-device-only -S``; per kernel: file, VGPRs, AGPRs, SGPRs, scratch bytes,
static LDS bytes, occupancy, instruction count, hash, demangled name without its argument list.  The hash covers the instructions
with symbol names and local labels normalised.  ``--diff`` compares two outputs by (file, name); each regex=replacement rewrites the
names of the first one beforehand ('winograd_conv_kernel<0>$=winograd_conv_kernel': a template list that shrank).
"""
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO = (("NumVgprs", "vgpr"), ("NumAgprs", "agpr"), ("TotalNumSgprs", "sgpr"), ("ScratchSize", "scratch"),
        ("LDSByteSize", "lds"), ("Occupancy", "occ"))
COLS = [c for _, c in INFO] + ["insts", "hash"]


def manifest(src, flags):
    asm = subprocess.run(["hipcc"] + flags + ["--offload-device-only", "-S", "-o", "-", src], check=True,
                         capture_output=True, text=True).stdout
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    rows = []
    # "<symbol>:" ... ".Lfunc_endN:" is the body; the "; Kernel info:" comment block that follows holds the resources
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^\t\.(?:text|section\t\.text)|\Z)", asm, re.M | re.S):
        sym, body, tail = m.groups()
        if sym not in kernels:
            continue
        insts = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if line.startswith(".LBB") and line.endswith(":"):
                line = re.sub(r"\.LBB\d+_", "L", line)
            elif not line or line.startswith(".") or line.endswith(":"):
                continue
            insts.append(re.sub(r"\b_Z\w+", "SYM", re.sub(r"\.LBB\d+_", "L", re.sub(r"\s+", " ", line))))
        n = sum(1 for i in insts if not i.endswith(":"))
        info = {c: re.search(r"^; %s: (\d+)" % k, tail, re.M).group(1) for k, c in INFO}
        h = hashlib.sha256("\n".join(insts).encode()).hexdigest()[:16]
        rows.append([sym] + [info[c] for _, c in INFO] + [str(n), h])
    names = subprocess.run(["/opt/rocm/llvm/bin/llvm-cxxfilt" if os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt") else "c++filt"],
                           input="\n".join(r[0] for r in rows), capture_output=True, text=True, check=True).stdout.split("\n")
    base = os.path.basename(src)
    return ["\t".join([base] + r[1:] + [nm]) for nm, r in sorted((short(nm), r) for r, nm in zip(rows, names))]


def short(name):
    """'void ffwm::(anonymous namespace)::k<1, true>(float const*, int)' -> 'k<1, true>'"""
    name = re.sub(r"^void |ffwm::(\(anonymous namespace\)::)?", "", name)
    depth = 0
    for i in range(len(name) - 1, -1, -1 if name.endswith(")") else 1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


def read(path, renames=()):
    out = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        for r in renames:
            f[-1] = re.sub(r.split("=", 1)[0], r.split("=", 1)[1], f[-1])
        if len(f) == len(COLS) + 2 and not line.startswith("#"):
            out[(f[0], f[-1])] = dict(zip(COLS, f[1:-1]))
    return out


def diff(a_path, b_path, renames):
    a, b = read(a_path, renames), read(b_path)
    for tag, keys in (("GONE    ", set(a) - set(b)), ("NEW     ", set(b) - set(a))):
        for k in sorted(keys):
            print("%s %s  %s" % ((tag,) + k))
    same = 0
    for k in sorted(set(a) & set(b)):
        if a[k]["hash"] == b[k]["hash"]:
            same += 1
            continue
        worse = any(int(b[k][c]) > int(a[k][c]) for c in ("scratch", "lds")) or int(b[k]["occ"]) < int(a[k]["occ"])
        print("%s  %s  %s  %s" % ("WORSE   " if worse else "CHANGED ", k[0], k[1], "  ".join(
            "%s %s->%s" % (c, a[k][c], b[k][c]) for c in COLS[:-1] if a[k][c] != b[k][c]) or "(same resources)"))
    print("# %d kernels before, %d after, %d with the same hash" % (len(a), len(b), same))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--diff"]:
        sys.exit(diff(args[1], args[2], args[3:]))
    root, args = (os.path.abspath(args[1]), args[2:]) if args[:1] == ["--root"] else (ROOT, args)
    sys.path.insert(0, root)
    from ffwm_amd.build import HIPCC_FLAGS
    srcs = args or sorted(glob.glob(os.path.join(root, "ffwm_amd", "csrc", "*.hip")))
    print("# file\t" + "\t".join(COLS) + "\tkernel")
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, len(srcs))) as ex:
        for lines in ex.map(lambda s: manifest(s, HIPCC_FLAGS), srcs):
            print("\n".join(lines))
