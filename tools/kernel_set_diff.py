"""The device kernels of two builds of the library, unit by unit: which kernels each object file holds, how many bytes of
machine code, and whether a kernel both builds hold has the same bytes over its symbol's range.  No GPU needed.

usage: kernel_set_diff.py OLD/topo_descriptors_amd/build NEW/topo_descriptors_amd/build [unit-prefix ...]
(unit prefixes default to the disc units: disc_wave_group disc_pair disc_wave).  Exit status 1 when NEW holds a kernel OLD
does not, or a kernel of both differs.

       kernel_set_diff.py --symbols OLD/.../build NEW/.../build [unit-prefix ...]
pairs kernels by name across all objects of each build directory (with prefixes: across the objects they select in
either), so a kernel that moved from one unit to another is compared with itself.  Same rules, same exit status."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj, tmp):
    """{kernel symbol: its machine code} of the gfx950 code object bundled into ``obj``."""
    fat, co = os.path.join(tmp, "unit.hipfb"), os.path.join(tmp, "unit.co")
    sections = subprocess.run([f"{LLVM}/llvm-readelf", "-SW", obj], check=True, capture_output=True, text=True).stdout
    if ".hip_fatbin" not in sections:
        return {}  # a unit of host code only
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "unit.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}",
                    "--unbundle"], check=True)
    text = None
    for line in subprocess.run([f"{LLVM}/llvm-readelf", "-SW", co], check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text = (int(f[0]), int(f[3], 16), int(f[4], 16))  # section index, address, file offset
    funcs, descriptors = {}, set()
    for line in subprocess.run([f"{LLVM}/llvm-readelf", "-sW", co], check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] == str(text[0]):
            funcs[f[7]] = (int(f[1], 16), int(f[2]))
        elif len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            descriptors.add(f[7][:-3])
    with open(co, "rb") as fh:
        image = fh.read()
    return {name: image[addr - text[1] + text[2]:addr - text[1] + text[2] + size] for name, (addr, size) in funcs.items()
            if name in descriptors}


def without_pc_offsets(code):
    """``code`` with the 32-bit literal of every ``s_getpc_b64 s[n:n+1]; s_add_u32 sn, sn, literal`` pair zeroed: the
    distance from the instruction to a table in .rodata, which moves when other kernels leave the unit."""
    words = list(struct.unpack(f"<{len(code) // 4}I", code))
    for k in range(len(words) - 2):
        if words[k] & 0xff80ffff == 0xbe801c00 and words[k + 1] & 0xff80ff00 == 0x8000ff00:
            words[k + 2] = 0
    return words


def demangled(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    if not filt or not names:
        return list(names)
    return subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]


def pooled(build_dir, prefixes, tmp):
    """{kernel: its machine code} over every object of ``build_dir`` whose name starts with one of ``prefixes``.  A kernel is
    named by its demangled symbol without the ``(anonymous namespace)::`` qualifiers: they stand for the unit, and differ
    between two builds when a kernel, or the type of one of its arguments, has moved to another unit or into a header."""
    pool = {}
    for unit in sorted(f for f in os.listdir(build_dir) if f.endswith(".o") and f.startswith(prefixes)):
        ks = kernels(os.path.join(build_dir, unit), tmp)
        for symbol, name in zip(ks, demangled(list(ks))):
            name = name.replace("(anonymous namespace)::", "")
            if name in pool and without_pc_offsets(pool[name]) != without_pc_offsets(ks[symbol]):
                name += f" [another one in {unit}]"  # (a template instance two units build is one kernel)
            pool.setdefault(name, ks[symbol])
    return pool


def main():
    by_symbol = sys.argv[1] == "--symbols"
    old_dir, new_dir = sys.argv[1 + by_symbol:3 + by_symbol]
    prefixes = tuple(sys.argv[3 + by_symbol:]) or (("",) if by_symbol else ("disc_wave_group", "disc_pair", "disc_wave"))
    units = ["all objects"] if by_symbol else sorted(f for f in os.listdir(old_dir) if f.endswith(".o") and f.startswith(prefixes))
    total = {"old": [0, 0], "new": [0, 0]}
    added, changed, moved, removed = [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            if by_symbol:
                old, new = pooled(old_dir, prefixes, tmp), pooled(new_dir, prefixes, tmp)
            else:
                old, new = kernels(os.path.join(old_dir, unit), tmp), kernels(os.path.join(new_dir, unit), tmp)
            for key, ks in (("old", old), ("new", new)):
                total[key][0] += len(ks)
                total[key][1] += sum(len(code) for code in ks.values())
            added += [(unit, k) for k in new if k not in old]
            removed += [(unit, k) for k in old if k not in new]
            differ = [k for k in new if k in old and new[k] != old[k]]
            moved += [(unit, k) for k in differ if without_pc_offsets(new[k]) == without_pc_offsets(old[k])]
            changed += [(unit, k) for k in differ if (unit, k) not in moved]
            print(f"{unit}: {len(old)} kernels, {sum(map(len, old.values()))} bytes -> {len(new)} kernels, {sum(map(len, new.values()))} bytes")
    print(f"all units: {total['old'][0]} kernels, {total['old'][1]} bytes -> {total['new'][0]} kernels, {total['new'][1]} bytes")
    print(f"removed {len(removed)}, added {len(added)}, kept with other bytes {len(changed)}, "
          f"kept with nothing but PC-relative offsets to .rodata moved {len(moved)}")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    for what, names in (("removed", removed), ("added", added), ("changed", changed), ("moved", moved)):
        for unit, k in names:
            print(what, unit, subprocess.run([filt, k], capture_output=True, text=True).stdout.strip() if filt else k)
    return 1 if added or changed else 0


if __name__ == "__main__":
    sys.exit(main())
