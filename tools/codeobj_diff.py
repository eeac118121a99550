"""Compares the gfx950 device code of two builds of libicap_hip.so kernel by kernel: llvm-objdump -d on the extracted
code objects, split per symbol, instruction addresses dropped (mnemonic, operands and encoding compared). Needs no GPU.

usage: python tools/codeobj_diff.py PARENT_LIB TREE_LIB OUT.txt"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([OBJDUMP, "--offloading", "lib.so"], check=True, capture_output=True, cwd=d)
        for o in sorted(os.listdir(d)):
            if not o.endswith("gfx950"):
                continue
            dis = subprocess.run([OBJDUMP, "-d", "-C", os.path.join(d, o)], check=True, capture_output=True, text=True).stdout
            sym = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
                if m:
                    sym = m.group(1)
                    assert sym not in out, sym
                    out[sym] = []
                elif sym is not None and line.startswith("\t"):
                    # "\tinsn operands   // 00000000B700: ENCODING": drop the address, keep the encoding
                    out[sym].append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())
    # the assembler pads the gap to the next (256-byte aligned) function with s_nop or zeros (objdump: "..."); which function comes next, and so
    # the length of the gap, depends on the order of instantiation: drop a function's trailing padding lines
    for v in out.values():
        while v and (v[-1].startswith("s_nop 0") or v[-1] == "..."):
            v.pop()
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
lines = []
ga, gb = sum("gemm" in s for s in a), sum("gemm" in s for s in b)
lines.append(f"symbols: parent {len(a)}, tree {len(b)}; with 'gemm' in the name: parent {ga}, tree {gb}")
lines.append(f"only in parent: {sorted(set(a) - set(b))}")
lines.append(f"only in tree: {sorted(set(b) - set(a))}")
diff = [s for s in sorted(set(a) & set(b)) if a[s] != b[s]]
lines.append("(each function without the padding that follows its last instruction)")
lines.append(f"instructions compared: {sum(len(v) for v in a.values())}")
lines.append(f"symbols whose instructions (mnemonic, operands, encoding) differ: {len(diff)}")
for s in diff:
    n = sum(x != y for x, y in zip(a[s], b[s])) + abs(len(a[s]) - len(b[s]))
    lines.append(f"  {s}: {len(a[s])} vs {len(b[s])} instructions, {n} differing lines")
    for x, y in list((x, y) for x, y in zip(a[s], b[s]) if x != y)[:5]:
        lines.append(f"    - {x}\n    + {y}")
open(sys.argv[3], "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
