"""Registers, LDS and SCRATCH of the kernels in a built object (stonkgs_amd/csrc/*.o): the .hip_fatbin section is unbundled
with the ROCm LLVM tools and the code object's metadata notes are read. A kernel whose hand-laid-out register file spills
still produces right answers - only slower (round 4: a few more scalars alive across the written-out K loop put 29-78
registers of every 256-wide gemm_a4 instance into scratch; FFN-up 144 -> 175 us) - so tests/test_host_cpu.py asserts on this.
  python tools/kernel_resources.py stonkgs_amd/csrc/gemm_a4.o"""
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
    can be compared kernel by kernel"""
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
        k["text"] = hashlib.sha1("\n".join(lines[k["name"]]).encode()).hexdigest()[:12]
    return out


if __name__ == "__main__":
    for k in kernel_resources(sys.argv[1]):
        print(f"{k['name'][:90]:90s} vgpr {k.get('vgpr', 0):3d} agpr {k.get('agpr', 0):3d} sgpr {k.get('sgpr', 0):3d} lds {k.get('lds', 0):6d} "
              f"scratch {k['scratch']:4d} spills v{k.get('vgpr_spill', 0)} s{k.get('sgpr_spill', 0)} text {k['text']}")
