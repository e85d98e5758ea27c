"""Are the kernels of two gfx950 code objects the same code?  (measurement aid; runs without a GPU)

    python tools/code_identity.py old new ['new name regex=old name' ...]

old / new: two builds of libx265hip.so, of one of its object files (csrc/_obj/x.o), or of a --cuda-device-only object.  One line per
kernel of `new`: its resource report (vgpr agpr sgpr vspill sspill lds scratch) against the old one and its disassembly (llvm-objdump -d,
addresses and encodings dropped) against that of the kernel of the same name - after the renames given - in `old`:
"identical", "identical but N pc-relative literals" where the only differing operands are the hexadecimal literals of s_add_u32 / s_addc_u32
(offsets from the pc to __constant__ data, which move with the layout of the object), or the first differing lines."""
import os
import re
import subprocess
import sys
import tempfile

from kernel_regs import code_objects

LLVM = "/opt/rocm/lib/llvm/bin/"
NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", n).replace("x265hip::", "").replace("void ", "") for n in out]


def kernels(path):
    """name -> (resource tuple, [instruction lines]) over every gfx950 code object of a library, an object file or an offload bundle"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(open(path, "rb").read())):
            elf = os.path.join(tmp, f"co{i}.elf")
            open(elf, "wb").write(co)
            out.update(kernels_of_elf(elf))
    return out


def kernels_of_elf(path):
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk)[1])
        res[re.search(r"\.name:\s+(\S+)", blk)[1]] = tuple(get(k) for k in NOTES)
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    code, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = code.setdefault(m[1], [])
        elif cur is not None and line.startswith("\t") and line.strip() != "...":          # "...": zero padding behind a kernel, elided by objdump
            cur.append(re.sub(r"\s*//.*", "", line).strip())
    syms = sorted(res)
    return {d: (res[s], code[s]) for s, d in zip(syms, demangle(syms))}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    renames = [r.rsplit("=", 1) for r in sys.argv[3:]]
    seen, bad = set(), 0
    literal = re.compile(r"^(s_addc?_u32 .*, )0x[0-9a-f]+$")
    for name in sorted(new):
        was = name
        for pat, rep in renames:
            was = re.sub(pat, rep, was)
        if was not in old:
            print(f"{name}: NOT in the old object (looked for {was})")
            bad += 1
            continue
        seen.add(was)
        (r0, c0), (r1, c1) = old[was], new[name]
        diff = [(a, b) for a, b in zip(c0, c1) if a != b]
        moved = [d for d in diff if literal.match(d[0]) and literal.match(d[1]) and literal.match(d[0])[1] == literal.match(d[1])[1]]
        if len(c0) != len(c1) or len(moved) != len(diff):
            verdict = f"DIFFERS ({len(c0)} -> {len(c1)} instructions): " + " | ".join(f"{a} -> {b}" for a, b in [d for d in diff if d not in moved][:4])
        else:
            verdict = "identical" + (f" but {len(moved)} pc-relative literals" if moved else "")
        same_res = "resources equal " + " ".join(map(str, r1)) if r0 == r1 else f"RESOURCES {r0} -> {r1}"
        bad += verdict.startswith("DIFFERS") or r0 != r1
        print(f"{name}{'  (was ' + was + ')' if was != name else ''}: {len(c1)} instructions, {verdict}; {same_res}")
    for name in sorted(set(old) - seen):
        print(f"{name}: only in the old object")
        bad += 1
    print(f"# {len(new)} kernels, {bad} that differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
