#!/usr/bin/env python3
"""Compare the kernels of two device assembly files: the acceptance check of a change that must not move generated code.

Both files come from `hipcc -S --cuda-device-only` with the Makefile's FLAGS (tools/isa_mix.py compiles the same way), one at the
commit before the change and one after:

    hipcc $FLAGS --cuda-device-only -S raycore.jl_amd/csrc/rc_drivers.hip -o after.s
    python3 tools/isa_diff.py before.s after.s [more pairs ...] > profiles/<change>_isa.txt

Each file is cut into kernels (.amdhsa_kernel symbols).  A kernel's instruction stream is its instruction lines with comments dropped,
local labels renumbered in order of appearance and mangled symbol names replaced by a placeholder.  Per kernel the report gives VGPRs,
SGPRs, private segment bytes, LDS bytes and the instruction count on both sides, and whether the streams are identical.  A kernel whose
name exists on one side only is paired with an unpaired kernel of the other side that has the same stream, if there is one (a rename).
The script only compares and counts.  Exit status 1 if any kernel differs or stays unpaired.
"""
import difflib
import re
import shutil
import subprocess
import sys


def kernels(path):
    """{mangled name: (metadata, normalised instruction stream)}"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", l)] if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"\s*\.amdhsa_kernel " + re.escape(name) + r"$", lines[i]))
        meta = {"lds": 0}
        for l in lines[end:end + 80]:
            m = re.match(r"\s*\.amdhsa_group_segment_fixed_size (\d+)", l)
            if m:
                meta["lds"] = int(m.group(1))
            m = re.match(r"\s*\.set " + re.escape(name) + r"\.(num_vgpr|numbered_sgpr|private_seg_size), (\d+)", l)
            if m:
                meta[m.group(1)] = int(m.group(2))
        labels, stream = {}, []
        for l in lines[start + 1:end]:
            t = l.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue  # comments, blank lines, directives
            t = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), t)
            t = re.sub(r"\b_Z\w+", "SYM", t)
            stream.append(re.sub(r"\s+", " ", t))
        meta["instructions"] = sum(1 for t in stream if not t.endswith(":"))
        out[name] = (meta, stream)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::", "", r)[:128] for n, r in zip(names, res)}  # (library kernels have names of several kB; the project's own fit)


def figures(meta):
    return "vgpr %3d  sgpr %3d  private %4d  lds %6d  instructions %5d" % (meta.get("num_vgpr", -1), meta.get("numbered_sgpr", -1),
                                                                          meta.get("private_seg_size", -1), meta["lds"], meta["instructions"])


def main():
    if len(sys.argv) < 3 or len(sys.argv) % 2 == 0:
        sys.exit(__doc__)
    bad = 0
    for before_path, after_path in zip(sys.argv[1::2], sys.argv[2::2]):
        before, after = kernels(before_path), kernels(after_path)
        pairs = [(n, n) for n in before if n in after]
        only_b, only_a = [n for n in before if n not in after], [n for n in after if n not in before]
        for b in list(only_b):  # renamed: the same stream under another name
            twin = next((a for a in only_a if after[a][1] == before[b][1]), None)
            if twin:
                pairs.append((b, twin)); only_b.remove(b); only_a.remove(twin)
        names = demangle(sorted(set(before) | set(after)))
        same = sum(1 for b, a in pairs if before[b] == after[a])
        print("== %s -> %s: %d kernels before, %d after, %d paired, %d identical in stream and figures" % (before_path, after_path, len(before), len(after), len(pairs), same))
        for b, a in sorted(pairs, key=lambda p: names[p[0]]):
            (mb, sb), (ma, sa) = before[b], after[a]
            verdict = "IDENTICAL" if sb == sa and mb == ma else ("identical stream, figures differ" if sb == sa else "DIFFERENT")
            print("%s  %s  %s" % (verdict, figures(ma), names[b] + ("" if a == b else "  ->  " + names[a])))
            if verdict != "IDENTICAL":
                bad += 1
                print("    before: " + figures(mb))
                for d in list(difflib.unified_diff(sb, sa, "before", "after", lineterm="", n=1))[:60]:
                    print("    " + d)
        for n in only_b:
            bad += 1
            print("ONLY BEFORE  %s  %s" % (figures(before[n][0]), names[n]))
        for n in only_a:
            bad += 1
            print("ONLY AFTER   %s  %s" % (figures(after[n][0]), names[n]))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
