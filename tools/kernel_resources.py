#!/usr/bin/env python3
"""Register / spill table of every kernel of one or more translation units (hipcc -Rpass-analysis=kernel-resource-usage), compiled
with the unit's own flags: the command line is the one csrc/Makefile's %.s rule prints (make -n), plus the remark flag.
usage: python tools/kernel_resources.py yfv2_block yfv2_stage2h ... [--filter=substring]"""
import re, shlex, subprocess, sys, os
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yolo_fastestv2_amd", "csrc")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
flt = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--filter=")]
for unit in args:
    dry = subprocess.run(["make", "-C", CSRC, "--no-print-directory", "-n", "-B", unit + ".s"], capture_output=True, text=True, check=True).stdout
    cmd = shlex.split([l for l in dry.splitlines() if " -S " in l][-1])
    cmd[cmd.index("-o") + 1] = "/dev/null"
    out = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC).stderr
    cur = None
    rows = {}
    for line in out.splitlines():
        m = re.search(r":\d+:\d+: remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip(); rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1); rows[cur][k.strip()] = v.strip()
    for name, r in rows.items():
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"\(.*", "", dem).replace("void ", "")
        if flt and not any(f in dem for f in flt):
            continue
        print("%-46s VGPR %3s AGPR %3s SGPR %3s  spill V %s S %s  scratch %s  occupancy %s  LDS %s" % (
            dem[:46], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("VGPRs Spill"), r.get("SGPRs Spill"),
            r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"), r.get("LDS Size [bytes/block]")))
