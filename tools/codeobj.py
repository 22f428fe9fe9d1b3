"""gfx950 code objects out of a HIP fat binary (.so / .o): the clang offload bundles of its .hip_fatbin section, uncompressed
(`__CLANG_OFFLOAD_BUNDLE__`, entries of (offset, size, triple)), and their disassembly per kernel (llvm-objdump -d).
usage: python tools/codeobj.py <lib.so> [kernel-name-substring]   -> per kernel: instructions, s_barrier count
       python tools/codeobj.py --diff <old .o/.so ...> -- <new .o/.so ...>
           the union of the kernels on each side, compared: symbols on one side only or twice on a side, kernels whose instruction listings differ, kernels
           whose resource metadata (RESOURCES, from the code objects' notes) differs.  Exit status 0 only if nothing differs: the check
           that a move of kernels between translation units left the device code alone."""
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count", ".kernarg_segment_size", ".max_flat_workgroup_size")


def code_objects(path, arch="gfx950"):
    blob = open(path, "rb").read()
    out = []
    for m in re.finditer(re.escape(MAGIC), blob):
        p = m.start()
        n, = struct.unpack_from("<Q", blob, p + 24)
        o = p + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, o)
            o += 24
            triple = blob[o:o + tl].decode()
            o += tl
            if triple.endswith(arch) and size:
                out.append(blob[p + off:p + off + size])
    return out


def kernels(path, arch="gfx950", match=None):
    """{mangled kernel symbol: [instruction text, ...]} over every code object of the file (match: only the code objects that
    contain this string, or one of these strings)"""
    res = {}
    names = None if match is None else [m.encode() for m in ([match] if isinstance(match, str) else match)]
    for elf in code_objects(path, arch):
        if names is not None and not any(n in elf for n in names):
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
            if m:
                cur = res.setdefault(m.group(1), [])
                continue
            if cur is None or not line.startswith("\t"):
                continue
            ins = line.split("//")[0].strip()
            if ins and ins != "...":        # (objdump's mark for a run of zero bytes: the padding behind a code object's last kernel)
                cur.append(ins)
    return res


def resources(path, arch="gfx950"):
    """{mangled kernel symbol: {key of RESOURCES: value}} from the AMDGPU metadata note of every code object of the file"""
    res = {}
    for elf in code_objects(path, arch):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            txt = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            if line.startswith("  - "):                      # the next entry of amdhsa.kernels
                cur = {}
                line = "    " + line[4:]
            m = re.match(r"^    (\.[a-z_]+):\s+(\S+)$", line)
            if cur is None or not m:
                continue
            if m.group(1) == ".name":
                res[m.group(2)] = cur
            elif m.group(1) in RESOURCES:
                cur[m.group(1)] = m.group(2)
    return res


def diff(old, new, out=sys.stdout):
    """compare the kernels of two sets of files; the number of differences found"""
    ndiff = 0

    def union(fn, paths, side):
        nonlocal ndiff
        res = {}
        for p in paths:
            for name, v in fn(p).items():
                if name in res and fn is kernels:            # a symbol emitted by two files of one side: only one copy could be compared
                    out.write(f"twice in {side}: {name} (again in {p})\n")
                    ndiff += 1
                res[name] = v
        return res
    ik, jk, ir, jr = union(kernels, old, "old"), union(kernels, new, "new"), union(resources, old, "old"), union(resources, new, "new")
    for side, a, b in (("old", ik, jk), ("new", jk, ik)):
        for name in sorted(set(a) - set(b)):
            out.write(f"only in {side}: {name}\n")
            ndiff += 1
    for name in sorted(set(ik) & set(jk)):
        if ik[name] != jk[name]:
            first = next((n for n, (x, y) in enumerate(zip(ik[name], jk[name])) if x != y), min(len(ik[name]), len(jk[name])))
            out.write(f"listing differs: {name}: {len(ik[name])} -> {len(jk[name])} instructions, first at {first}\n")
            ndiff += 1
        if ir.get(name) != jr.get(name):
            out.write(f"resources differ: {name}: {ir.get(name)} -> {jr.get(name)}\n")
            ndiff += 1
    out.write(f"{len(ik)} kernels, {sum(map(len, ik.values()))} instructions (old); {len(jk)} kernels, {sum(map(len, jk.values()))} instructions (new); "
              f"{ndiff} differences\n")
    return ndiff


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        if "--" not in sys.argv:
            sys.exit(__doc__)
        sep = sys.argv.index("--")
        sys.exit(1 if diff(sys.argv[2:sep], sys.argv[sep + 1:]) else 0)
    ks = kernels(sys.argv[1], match=sys.argv[2] if len(sys.argv) > 2 else None)
    for name, ins in ks.items():
        if len(sys.argv) > 2 and sys.argv[2] not in name:
            continue
        print(len(ins), sum(i.startswith("s_barrier") for i in ins), name[:150])
