#!/usr/bin/env python
"""Do two builds of the library hold the same device code?   python tools/codeobj_diff.py A.so B.so

Extracts the gfx950 code objects of both libraries (llvm-objdump --offloading, as tests/test_no_spills.py does), prints a SHA-256
of each pair and `identical` or `different`; for a differing pair, what differs and the kernels whose machine code or descriptor
notes (registers, LDS, scratch, kernarg size) differ.  Exit status 0 only when every pair is identical.  No GPU needed.

The digest covers every section's bytes (code, kernel descriptors, metadata notes, data), every symbol's (name, offset in its
section, size, type, binding, section) and the dynamic tags.  Left out is what `__hip_cuid_<hash>` moves: hipcc derives that
symbol's hex digits, 16 or fewer, from its command line, and audio_amd/_build.py compiles into a file named after the process
id, so two compilations of ONE source differ in the name, its length (DT_STRSZ), and the order and hash tables of the symbol
sections -- .dynsym, .symtab, .dynstr, .strtab, .hash, .gnu.hash are compared as symbol lists, .dynamic as tags without STRSZ."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
NOTES = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
         "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")
AS_LISTS = (".dynsym", ".symtab", ".dynstr", ".strtab", ".hash", ".gnu.hash", ".dynamic")


def tool(name, *args, **kw):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True, **kw).stdout


def bundles(so, d):
    """The gfx950 code objects of the library, extracted into directory d: one per source it was linked from."""
    os.makedirs(d)
    shutil.copy(so, os.path.join(d, "lib.so"))
    tool("llvm-objdump", "--offloading", "lib.so", cwd=d)
    return sorted((f for f in os.listdir(d) if "gfx950" in f), key=lambda f: int(f.split(".")[2]))


class CodeObject:
    def __init__(self, path):
        with open(path, "rb") as f:
            raw = f.read()
        self.parts, place = {}, {}                       # what is compared, by name; section number -> (name, address, file offset)
        for line in tool("llvm-readelf", "-S", "-W", path).splitlines():
            m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s", line)
            if m and m.group(3) != "NULL":
                name, (addr, off, size) = m.group(2), (int(m.group(i), 16) for i in (4, 5, 6))
                place[m.group(1)] = (name, addr, off)
                if name not in AS_LISTS:
                    self.parts[name] = b"%d:" % size + (b"" if m.group(3) == "NOBITS" else raw[off:off + size])
        symbols, self.code = set(), {}                   # function -> machine code
        for line in tool("llvm-readelf", "-s", "--dyn-syms", "-W", path).splitlines():
            w = line.split()
            if len(w) == 8 and w[0][:-1].isdigit():
                sec, addr, off = place.get(w[6], (w[6], 0, 0))
                symbols.add((re.sub(r"^__hip_cuid_[0-9a-f]+$", "__hip_cuid_", w[7]), int(w[1], 16) - addr, w[2], w[3], w[4], w[5], sec))
                if w[3] == "FUNC" and w[6] in place:
                    self.code[w[7]] = raw[int(w[1], 16) - addr + off:][:int(w[2])]
        self.parts["symbols"] = repr(sorted(symbols)).encode()
        self.parts["dynamic tags"] = "\n".join(l for l in tool("llvm-readelf", "-d", path).splitlines()
                                               if l.startswith("  0x") and "STRSZ" not in l).encode()
        self.notes, name = {}, None                      # kernel -> descriptor notes
        for line in tool("llvm-readelf", "--notes", path).splitlines():
            m = re.match(r"\s*\.(name|%s):\s+(\S+)" % "|".join(NOTES), line)
            if m and m.group(1) == "name":
                name = m.group(2)
            elif m and name:
                self.notes.setdefault(name, {})[m.group(1)] = m.group(2)
        self.digest = hashlib.sha256(b"".join(k.encode() + b"\0" + self.parts[k] for k in sorted(self.parts))).hexdigest()


def main(a, b):
    with tempfile.TemporaryDirectory() as d:
        da, db = os.path.join(d, "a"), os.path.join(d, "b")
        fa, fb = bundles(a, da), bundles(b, db)
        if not fa or fa != fb:
            print("code objects: %r against %r" % (fa, fb))
            return 1
        bad = 0
        for f in fa:
            x, y = CodeObject(os.path.join(da, f)), CodeObject(os.path.join(db, f))
            print("%2s %s %s %s" % (f.split(".")[2], x.digest, y.digest, "identical" if x.digest == y.digest else "different"))
            if x.digest == y.digest:
                continue
            bad += 1
            print("     differ: " + ", ".join(k for k in sorted(set(x.parts) | set(y.parts)) if x.parts.get(k) != y.parts.get(k)))
            for k in sorted(set(x.code) | set(y.code)):
                if k not in x.code or k not in y.code:
                    print("     %s: only in %s" % (k, a if k in x.code else b))
                    continue
                what = ["code (%d -> %d bytes)" % (len(x.code[k]), len(y.code[k]))] if x.code[k] != y.code[k] else []
                nx, ny = x.notes.get(k, {}), y.notes.get(k, {})
                what += ["%s %s -> %s" % (n, nx.get(n), ny.get(n)) for n in NOTES if nx.get(n) != ny.get(n)]
                if what:
                    print("     %s: %s" % (k, ", ".join(what)))
        print("%d of %d code objects differ" % (bad, len(fa)))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]) if len(sys.argv) == 3 else __doc__)
