#!/usr/bin/env python
"""Device-code identity of two builds of the library, for refactors that must not change a kernel:
   python tools/isa_diff.py <build dir A> <build dir B>      (e.g. two copies of ao_amd/csrc/build)
Every *.o of both directories is unbundled (llvm-objdump --offloading), its gfx950 code object disassembled and its
kernel metadata read (llvm-readelf --notes).  Compared over the whole library, whichever object a function sits in:
  * the set of device function symbols,
  * per symbol the instruction text (addresses and encodings stripped; branch targets are relative to their symbol;
    pc-relative references to device data and the fill between functions normalised, see functions()),
  * per kernel vgpr / sgpr count, LDS, scratch and kernarg sizes.
A symbol that several objects emit (a static kernel defined in a header) is compared as the set of its distinct copies:
one copy where every unit is built alike, two where a unit has flags of its own (augment.o: contraction off).
Prints the differing symbols and exits 1 if there are any.  Reads nothing outside the two directories (the unbundled
code objects go to a scratch subdirectory of each, removed again)."""
import glob, os, re, shutil, subprocess, sys

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), cwd=cwd, check=True, capture_output=True, text=True).stdout


def data_symbols(code_object):
    """(address, size, name) of the data objects of a code object"""
    out = []
    for line in run("llvm-readelf", "-s", "--wide", code_object).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "OBJECT" and f[2].isdigit() and int(f[2]) > 0:
            out.append((int(f[1], 16), int(f[2]), f[7]))
    return out


def functions(code_object):
    """symbol -> instruction text, with what depends on where the linker put things taken out:
    a 32-bit literal of a scalar add (the s_add_u32 behind s_getpc_b64: the only way an address is formed) that, added to the
    address of its own instruction, lands inside a data object of the code object is a pc-relative reference to it (every
    unit has its own copy of the header's static device data, at its own distance from the code) and is written as
    <object+offset>; any other literal is compared as it stands (a vector instruction's constant such as 0xfffffe00 lands in
    some kernel descriptor as soon as the unit is large enough).  The fill behind the end of a function (the run of one
    repeated line that closes it, longest behind the last function of an object) is dropped."""
    data = data_symbols(code_object)
    out, name = {}, None
    for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", code_object).splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip() not in ("", "...") and not line.startswith("Disassembly"):  # ("...": zero fill)
            text, _, comment = line.partition("//")
            lit, at = re.search(r"\b0x([0-9a-f]{8})\b", text), re.match(r"\s*([0-9A-Fa-f]+):", comment)
            if lit and at and text.split()[0] in ("s_add_u32", "s_addc_u32"):
                v = int(lit.group(1), 16)
                target = int(at.group(1), 16) + (v - (1 << 32) if v >> 31 else v)
                for addr, size, sym in data:
                    if addr <= target < addr + size:
                        text = text.replace(lit.group(0), "<%s+%d>" % (sym, target - addr))
            out[name].append(text.strip())
    for lines in out.values():
        if len(lines) > 1 and lines[-1] == lines[-2]:
            last = lines[-1]
            while lines and lines[-1] == last:
                lines.pop()
    return {k: "\n".join(v) for k, v in out.items()}


def metadata(code_object):
    """kernel symbol -> the META fields"""
    out, cur = {}, None
    for line in run("llvm-readelf", "--notes", code_object).splitlines():
        m = re.match(r"^\s*(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        indent = len(line) - len(line.lstrip())
        if m.group(1) and indent <= 4 and m.group(2) in (".agpr_count", ".args"):  # first key of a kernel entry
            cur = {}
        if cur is None or indent > 6 or (m.group(1) and m.group(2) not in (".agpr_count", ".args")):
            continue  # (deeper: the entries of .args)
        cur[m.group(2)] = m.group(3).strip("'\"")
        if m.group(2) == ".symbol":
            out[cur[".symbol"][:-3] if cur[".symbol"].endswith(".kd") else cur[".symbol"]] = cur
    return {k: tuple(v.get(f) for f in META) for k, v in out.items()}


def library(build_dir):
    """symbol -> set of (instruction text, metadata) over all objects"""
    lib = {}
    tmp = os.path.join(build_dir, "isa_diff.tmp")
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    try:
        for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
            shutil.copy(obj, tmp)
            run("llvm-objdump", "--offloading", os.path.basename(obj), cwd=tmp)
            for co in glob.glob(os.path.join(tmp, os.path.basename(obj) + ".*gfx950*")):
                meta = metadata(co)
                for sym, text in functions(co).items():
                    lib.setdefault(sym, set()).add((text, meta.get(sym)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return lib


def main():
    a, b = library(sys.argv[1]), library(sys.argv[2])
    bad = []
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            bad.append((sym, "only in " + (sys.argv[1] if sym in a else sys.argv[2])))
        elif a[sym] != b[sym]:
            if len(a[sym]) != 1 or len(b[sym]) != 1:
                bad.append((sym, "%d distinct copies -> %d, not the same ones" % (len(a[sym]), len(b[sym]))))
                continue
            (ta, ma), (tb, mb) = next(iter(a[sym])), next(iter(b[sym]))
            bad.append((sym, "instructions differ" if ta != tb else "metadata %s -> %s" % (ma, mb)))
    kernels = sum(1 for s in a if next(iter(a[s]))[1] is not None)
    for sym, why in bad:
        print("DIFF %s: %s" % (sym, why))
    print("symbols compared: %d (%d kernels with metadata), differing: %d" % (len(set(a) | set(b)), kernels, len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
