#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of one translation unit: which kernels exist in both, whether their instruction
streams are identical, and the register / scratch figures of the kernels only the second build has.  No GPU: the objects are what
`make lib` (or hipcc -c) leaves on the build machine.

usage: kernel_diff.py PARENT.o NEW.o [--base-of OLD=NEW]
  --base-of   a substitution on the demangled name of a NEW kernel that names the kernel to compare its registers with
              (e.g. ', true, true>=, true, false>' : the shared-state instantiation an RG instantiation derives from)
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def device_elf(obj, tmp):
    obj = os.path.abspath(obj)
    d = tempfile.mkdtemp(dir=tmp)
    link = os.path.join(d, "x.o")
    os.symlink(obj, link)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", link], cwd=d, stdout=subprocess.DEVNULL)
    got = [f for f in os.listdir(d) if "amdgcn" in f]
    assert len(got) == 1, got
    return os.path.join(d, got[0])


def kernels(elf):
    """{mangled name: (sha1 of the instruction text, instruction count)} and {mangled name: metadata dict}"""
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", elf], text=True)
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip()) or re.match(r"^[0-9a-f]+ <(\S+)>:$", line.strip())
        if m:
            cur = m.group(1)
            code[cur] = []
            continue
        if cur is not None and line.strip():
            # branch targets carry absolute addresses in the comment: keep the instruction, drop the comment
            code[cur].append(re.sub(r"\s*//.*$", "", line.strip()))
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], text=True)
    meta, cur = {}, None
    for line in notes.splitlines():                     # one block per kernel: "  - .agpr_count: ..." opens it, keys at indent 4
        if line.startswith("  - ."):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    \.(\w+):\s*(.*)$", line)
        if cur is None or not m:
            continue
        cur[m.group(1)] = m.group(2).strip().strip("'")
        if m.group(1) == "name":
            meta[cur["name"]] = cur
    by_symbol = meta
    return {k: (hashlib.sha1("\n".join(v).encode()).hexdigest(), len(v)) for k, v in code.items() if k in by_symbol}, by_symbol


def demangle(names):
    # (_Float16 / __bf16 template arguments: binutils' c++filt may not know DF16_ / DF16b — spell them as named types first)
    plain = [n.replace("DF16_", "8_Float16").replace("DF16b", "6__bf16") for n in names]
    out = subprocess.run(["c++filt"] + plain, capture_output=True, text=True).stdout.split("\n")
    short = lambda n: re.sub(r"\(spatten::.*$", "", n).replace("spatten::", "").replace("void ", "")
    return {a: short(b) for a, b in zip(names, out)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    base_of = None
    if "--base-of" in sys.argv:
        base_of = sys.argv[sys.argv.index("--base-of") + 1].split("=", 1)
        args.remove("=".join(base_of))
    with tempfile.TemporaryDirectory() as tmp:
        (c0, m0), (c1, m1) = (kernels(device_elf(a, tmp)) for a in args)
    names = demangle(sorted(set(c0) | set(c1)))
    both = sorted(set(c0) & set(c1))
    same = [k for k in both if c0[k] == c1[k]]
    regs = lambda m: (m.get("vgpr_count"), m.get("sgpr_count"), m.get("agpr_count"), m.get("private_segment_fixed_size"),
                      m.get("group_segment_fixed_size"))
    same_regs = [k for k in both if regs(m0[k]) == regs(m1[k])]
    print(f"kernels in the parent build: {len(c0)}; in the new build: {len(c1)}; in both: {len(both)}")
    print(f"  gone from the new build: {len(set(c0) - set(c1))}")
    print(f"  instruction stream identical (sha1 of the disassembly without addresses): {len(same)} of {len(both)}")
    print(f"  VGPR / SGPR / AGPR / scratch / LDS figures identical: {len(same_regs)} of {len(both)}")
    print(f"  instructions over the kernels in both: {sum(c0[k][1] for k in both)} (parent), {sum(c1[k][1] for k in both)} (new)")
    ks = sorted({(m0[k].get("kernarg_segment_size"), m1[k].get("kernarg_segment_size")) for k in both})
    print(f"  kernarg segment bytes (parent, new) over the kernels in both: {ks}")
    for k in both:
        if k not in same or k not in same_regs:
            print(f"  CHANGED {names[k]}: {c0[k][1]} -> {c1[k][1]} instructions, regs {regs(m0[k])} -> {regs(m1[k])}")
    new = sorted(set(c1) - set(c0), key=lambda k: names[k])
    print(f"new kernels: {len(new)}")
    rev = {v: k for k, v in names.items() if k in c1}
    for k in new:
        line = f"  {names[k]}: {c1[k][1]} instructions, VGPR {m1[k].get('vgpr_count')} SGPR {m1[k].get('sgpr_count')} " \
               f"scratch {m1[k].get('private_segment_fixed_size')} LDS {m1[k].get('group_segment_fixed_size')}"
        if base_of:
            b = rev.get(names[k].replace(base_of[0], base_of[1]))
            if b and b != k:
                line += f" | base: {c1[b][1]} instructions, VGPR {m1[b].get('vgpr_count')} SGPR {m1[b].get('sgpr_count')} " \
                        f"scratch {m1[b].get('private_segment_fixed_size')}"
            else:
                line += " | base: not found"
        print(line)
    scr = [names[k] for k in c1 if int(m1[k].get("private_segment_fixed_size") or 0) != 0]
    print(f"kernels of the new build with scratch: {len(scr)}" + ("" if not scr else ": " + "; ".join(scr)))


if __name__ == "__main__":
    main()
