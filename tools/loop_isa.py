#!/usr/bin/env python3
"""On the CPU: per kernel of a unit's device assembly (make -C yolo_fastestv2_amd/csrc UNIT.s) the registers, scratch bytes and waves
per SIMD the compiler reports, and the static instruction mix of its largest innermost loop (the steady-state row loop of the
streaming kernels): VALU (every v_* that is not an MFMA or an accumulation-register move), MFMA, LDS, buffer / global memory, scalar.
A block belongs to a loop by the compiler's own "in Loop: Header=" comments; side blocks the compiler moved behind the loop count too.
usage: python tools/loop_isa.py FILE.s [kernel-name-substring ...]"""
import re
import subprocess
import sys


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "acc_move"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "scalar"
    return "other"


def kernels(path):
    """-> [(symbol, [lines])] for every .type NAME,@function body"""
    lines = open(path).read().splitlines()
    out, cur, name = [], None, None
    for ln in lines:
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", ln)
        if m and cur is None and not ln.startswith(".L"):
            name, cur = m.group(1), []
            continue
        if cur is not None:
            cur.append(ln)
            if re.match(r"^\s*; Occupancy:", ln):            # the resource comments follow .end_amdhsa_kernel
                out.append((name, cur))
                cur = None
    return out


def analyse(body):
    info = {}
    for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("waves_per_simd", r"; Occupancy: (\d+)")):
        for ln in body:
            m = re.search(pat, ln)
            if m:
                info[key] = int(m.group(1))
    # blocks: label -> (loop header or None, instruction mnemonics)
    loops, header = {}, None
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", ln)
        if m:
            c = m.group(2) or ""
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", c)
            if "This Inner Loop Header" in c:
                header = m.group(1)[2:]
            elif h:
                header = h.group(1)
            else:
                header = None
            continue
        s = ln.strip()
        if header is None or not s or s.startswith((";", ".")):
            continue
        loops.setdefault(header, []).append(s.split()[0])
    if loops:
        h, ops = max(loops.items(), key=lambda kv: len(kv[1]))
        mix = {}
        for op in ops:
            mix[classify(op)] = mix.get(classify(op), 0) + 1
        info["loop"] = h
        info["loop_instructions"] = len(ops)
        info["mix"] = mix
    return info


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    for name, body in kernels(path):
        pretty = demangle(name)
        if pats and not any(p in pretty for p in pats):
            continue
        i = analyse(body)
        if "vgprs" not in i:
            continue
        mix = i.get("mix", {})
        print("%-40s vgprs %3d agprs %3d scratch %d waves/SIMD %d | loop %-8s %5d instr: valu %4d mfma %3d acc_move %3d lds %3d vmem %3d scalar %3d other %d" % (
            pretty.split("(")[0][:40], i["vgprs"], i.get("agprs", 0), i["scratch"], i["waves_per_simd"], i.get("loop", "-"), i.get("loop_instructions", 0),
            mix.get("valu", 0), mix.get("mfma", 0), mix.get("acc_move", 0), mix.get("lds", 0), mix.get("vmem", 0), mix.get("scalar", 0), mix.get("other", 0)))


if __name__ == "__main__":
    main()
