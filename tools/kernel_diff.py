#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of host objects:  tools/kernel_diff.py OLD.o [OLD.o ...] -- NEW.o [NEW.o ...]

For a refactor that moves kernels between translation units without meaning to change them.  From every object the device
code object is taken out (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle) and, per kernel symbol,
three things are read: its size (llvm-readelf -sW), its metadata record (llvm-readelf --notes: register and spill counts,
segment sizes, workgroup size, arguments) and its instruction text (llvm-objdump -d).  Prints the kernels that are missing on
one side, sit in more than one object of a side, or differ in any of the three; exit status 0 when there are none."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def device_object(obj, tmp):
    fat = os.path.join(tmp, "fatbin")
    co = os.path.join(tmp, "%d.co" % len(os.listdir(tmp)))
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
    return co


def kernels_of(obj, tmp):
    """{kernel: (size, metadata text, instruction text)} of one host object"""
    co = device_object(obj, tmp)
    sizes, start, descriptors = {}, {}, set()
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            sizes[f[7]], start[f[7]] = int(f[2]), int(f[1], 16)
        if len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            descriptors.add(f[7][:-3])
    meta = {}
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    body = notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0] if "amdhsa.kernels:" in notes else ""
    for rec in re.split(r"^  - ", body, flags=re.M)[1:]:
        meta[re.search(r"^\s*\.name:\s+(\S+)", rec, flags=re.M).group(1)] = rec.replace("...", "").rstrip()
    text, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = m.group(1)
            text[cur] = []
        elif cur in sizes:  # an instruction: "text // ADDRESS: ENCODING"; the address only says where the kernel sits in its object
            m = re.search(r"//\s*([0-9A-Fa-f]+):", line)
            if m and int(m.group(1), 16) < start[cur] + sizes[cur]:  # (behind a unit's last kernel comes padding)
                text[cur].append(line.strip().replace(m.group(0), "//"))
    return {k: (sizes[k], meta.get(k, ""), "\n".join(text.get(k, []))) for k in sizes if k in descriptors}


def side(objs, tmp):
    out, dup = {}, []
    for o in objs:
        for k, v in kernels_of(o, tmp).items():
            if k in out:
                dup.append(k)
            out[k] = v
    return out, dup


def main(argv):
    if "--" not in argv:
        sys.exit(__doc__)
    old, new = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    with tempfile.TemporaryDirectory() as tmp:
        a, dup_a = side(old, tmp)
        b, dup_b = side(new, tmp)
    bad = 0
    for k in dup_a:
        print("in more than one old object:", k); bad += 1
    for k in dup_b:
        print("in more than one new object:", k); bad += 1
    for k in sorted(set(a) - set(b)):
        print("missing in the new objects:", k); bad += 1
    for k in sorted(set(b) - set(a)):
        print("only in the new objects:", k); bad += 1
    for k in sorted(set(a) & set(b)):
        what = [n for n, x, y in zip(("size", "metadata", "instructions"), a[k], b[k]) if x != y]
        if what:
            print("differs (%s): %s" % (", ".join(what), k)); bad += 1
    print("%d kernels old, %d new, %d compared, %d findings" % (len(a), len(b), len(set(a) & set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
