"""Per-symbol comparison of the gfx950 code objects of two builds of the library.
   python tools/code_object_diff.py OLD.so NEW.so
Unbundles each library's .hip_fatbin, disassembles it and compares, symbol by symbol, the instruction text
(addresses dropped: the order of the kernels in the object follows their first use in the host code; a pc-relative
target is named by function + offset, or by section + offset when it lies outside the code).  Prints
the symbol counts, the symbols on one side only and the ones whose bodies differ; exit status 1 when any do."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def fatbin(lib):
    """The bytes of the ELF section .hip_fatbin (found as _build.code_object_sha finds it)."""
    elf = open(lib, "rb").read()
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    stroff = sec[shstrndx][4]
    for name, _t, _f, _a, off, size in sec:
        if elf[stroff + name:elf.index(b"\0", stroff + name)] == b".hip_fatbin":
            return elf[off:off + size]
    sys.exit(f"{lib}: no .hip_fatbin section")


def symbols(lib, tmp, tag):
    """{symbol: [instruction text]} of the library's gfx950 code object."""
    fb, co = os.path.join(tmp, tag + ".hipfb"), os.path.join(tmp, tag + ".co")
    open(fb, "wb").write(fatbin(lib))
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fb}", f"--output={co}"], check=True)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                          capture_output=True, text=True).stdout
    out, cur, starts, prev = {}, None, [], ""
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(2), [])
            starts.append((int(m.group(1), 16), m.group(2)))
        elif cur is not None and line.strip() == "...":
            continue  # objdump's mark for the zero padding up to the next symbol's alignment: not part of the body
        elif cur is not None and line.strip():
            ins, _, note = line.partition("//")
            ins = re.sub(r"\s+", " ", ins).strip()
            # s_getpc_b64 + s_add_u32 literal: a pc-relative address, which moves with the kernel; compare its target
            lit = re.match(r"(s_add_u32 \S+ \S+) (0x[0-9a-f]+)$", ins) if prev.startswith("s_getpc_b64") else None
            if lit:
                cur.append((lit.group(1), int(note.split(":")[0], 16) + int(lit.group(2), 16)))
            else:
                cur.append(ins)
            prev = ins
    # (a target inside a function as function + offset, anything else -- .rodata, .got -- as section + offset: a
    # table keeps its place in its section when kernels are added, while its address moves with the code before it)
    starts.sort()
    sections = []
    for line in subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-h", co], check=True, capture_output=True,
                               text=True).stdout.splitlines():
        f = line.split()
        if len(f) >= 4 and f[0].isdigit() and f[1].startswith("."):
            sections.append((f[1], int(f[3], 16), int(f[2], 16)))  # name, address, size
    def place(addr):
        inside = [(a, s) for a, s in starts if a <= addr]
        if inside and addr < starts[-1][0]:
            return f"{inside[-1][1]}+{addr - inside[-1][0]:#x}"
        for name, base, size in sections:
            if name != ".text" and base <= addr < base + size:
                return f"{name}+{addr - base:#x}"
        return f"@{addr:#x}"
    return {s: [i if isinstance(i, str) else f"{i[0]} {place(i[1])}" for i in body] for s, body in out.items()}


with tempfile.TemporaryDirectory() as tmp:
    old, new = symbols(sys.argv[1], tmp, "old"), symbols(sys.argv[2], tmp, "new")
gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
differ = sorted(s for s in set(old) & set(new) if old[s] != new[s])
print(f"{len(old)} -> {len(new)} symbols, {len(gone)} only in old, {len(added)} only in new, {len(differ)} bodies differ")
for title, names in (("only in old", gone), ("only in new", added), ("differs", differ)):
    for s in names:
        print(f"  {title}: {s}" + (f" ({len(old[s])} -> {len(new[s])} instructions)" if title == "differs" else ""))
sys.exit(1 if gone or added or differ else 0)
