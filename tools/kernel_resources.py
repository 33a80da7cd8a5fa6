"""Registers, LDS and SCRATCH of the kernels in a built object (stonkgs_amd/csrc/*.o): the .hip_fatbin section is unbundled
with the ROCm LLVM tools and the code object's metadata notes are read. A kernel whose hand-laid-out register file spills
still produces right answers - only slower (round 4: a few more scalars alive across the written-out K loop put 29-78
registers of every 256-wide gemm_a4 instance into scratch; FFN-up 144 -> 175 us) - so tests/test_host_cpu.py asserts on this.
  python tools/kernel_resources.py stonkgs_amd/csrc/gemm_a4.o
With two objects - the same source built from two commits - every kernel gets one of three verdicts (`compare`):
  python tools/kernel_resources.py parent/norm.o stonkgs_amd/csrc/norm.o [--diff SUBSTRING]"""
import collections
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_resources(obj):
    """[{name, vgpr, agpr, sgpr, lds, scratch, vgpr_spill, sgpr_spill, text}] for every kernel of the gfx950 code object in
    `obj`; text = a hash of the kernel's instructions (llvm-objdump -d without encodings and addresses), so that two builds
    can be compared kernel by kernel; listing = those instructions, one per line"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        # (with an output file: without one llvm-objcopy rewrites `obj` in place, and make then links again)
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "copy.o")], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    keys = {".name": "name", ".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds",
            ".private_segment_fixed_size": "scratch", ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill"}
    out = []
    for line in notes.splitlines():
        m = re.match(r"^  (-| ) (\.\w+):\s+(\S+)\s*$", line)   # a kernel's own keys ("- " opens the next kernel; .args lie deeper)
        if m and m.group(1) == "-":
            out.append({})
        if m and out and m.group(2) in keys:
            out[-1][keys[m.group(2)]] = m.group(3) if m.group(2) == ".name" else int(m.group(3))
    out = [k for k in out if "scratch" in k]
    # a kernel's instructions: from its symbol to the next kernel's (the labels of inline assembly are symbols too: dropped)
    lines = {k["name"]: [] for k in out}
    cur = None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = lines.get(m.group(1), cur)
        elif cur is not None and line.strip() not in ("", "..."):   # (padding behind an object's last kernel)
            # (without the address comment and the per-block number that %= gives the written-out loops' labels)
            cur.append(re.sub(r"\b(L_\w+?)_\d+$", r"\1", re.sub(r"\s*//.*", "", line)))
    for k in out:
        k["listing"] = [" ".join(x.split()) for x in lines[k["name"]]]
        k["text"] = hashlib.sha1("\n".join(lines[k["name"]]).encode()).hexdigest()[:12]
    return out


def compare(parent_obj, branch_obj):
    """[(name, verdict, parent kernel, branch kernel)] over the kernels of both objects (None where one lacks it):
      identical  the instruction hashes agree
      same work  they differ, but the instruction count and the count of every mnemonic are equal, LDS bytes and scratch
                 are equal, no VGPR spills, and VGPRs, SGPRs and SGPR spills are no higher than the parent's
      differs    anything else
    Whole listings and counts are compared; no particular instruction is looked for."""
    a = {k["name"]: k for k in kernel_resources(parent_obj)}
    b = {k["name"]: k for k in kernel_resources(branch_obj)}
    out = []
    gone = {a[n]["text"]: n for n in a if n not in b}
    for name in list(a) + [n for n in b if n not in a]:
        p, q = a.get(name), b.get(name)
        if p is None and q["text"] in gone:   # a kernel that only changed its name (became a template's instance)
            continue
        if q is None and p["text"] in {b[n]["text"] for n in b if n not in a}:
            q = next(b[n] for n in b if n not in a and b[n]["text"] == p["text"])
            name, verdict = f"{name} -> {q['name']}", "identical"
        elif p is None or q is None:
            verdict = "differs"
        elif p["text"] == q["text"]:
            verdict = "identical"
        else:
            def mix(k):
                return collections.Counter(x.split()[0] for x in k["listing"])
            g = lambda k, key: k.get(key, 0)
            same = (len(p["listing"]) == len(q["listing"]) and mix(p) == mix(q)
                    and g(p, "lds") == g(q, "lds") and g(p, "scratch") == g(q, "scratch")
                    and g(p, "vgpr_spill") == 0 and g(q, "vgpr_spill") == 0
                    and all(g(q, key) <= g(p, key) for key in ("vgpr", "agpr", "sgpr", "sgpr_spill")))
            verdict = "same work" if same else "differs"
        out.append((name, verdict, p, q))
    return out


if __name__ == "__main__":
    args, want = sys.argv[1:], None
    if "--diff" in args:   # the listings' diff for the kernels whose name holds SUBSTRING
        want = args[args.index("--diff") + 1]
        del args[args.index("--diff"):args.index("--diff") + 2]
    if len(args) == 2:
        for name, verdict, p, q in compare(args[0], args[1]):
            n = lambda k: len(k["listing"]) if k else 0
            # (for a "same work" kernel: whether the two listings also have the same opcodes in the same ORDER, that is,
            # differ in operands alone - what a difference inside a per-row loop must satisfy)
            ops = lambda k: [x.split()[0] for x in k["listing"]]
            order = "" if verdict != "same work" else ("  operands only" if ops(p) == ops(q) else "  order differs")
            print(f"{name[:100]:100s} {verdict:9s} insns {n(p):5d} -> {n(q):5d}{order}")
            if want and want in name and p and q and verdict != "identical":
                print("\n".join(difflib.unified_diff(p["listing"], q["listing"], "parent", "branch", lineterm="", n=1)))
        sys.exit(0)
    for k in kernel_resources(sys.argv[1]):
        print(f"{k['name'][:90]:90s} vgpr {k.get('vgpr', 0):3d} agpr {k.get('agpr', 0):3d} sgpr {k.get('sgpr', 0):3d} lds {k.get('lds', 0):6d} "
              f"scratch {k['scratch']:4d} spills v{k.get('vgpr_spill', 0)} s{k.get('sgpr_spill', 0)} text {k['text']}")
