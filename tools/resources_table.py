"""build/resources.txt (make resources) as one line per kernel: name | SGPRs VGPRs AGPRs scratch occupancy sgpr-spill vgpr-spill LDS | units.
A kernel compiled into several units is one line when its numbers agree in all of them (they always have); names over 150 characters
are cut and carry a hash of the whole name.
usage: make -C rivulus_amd/csrc resources; python3 tools/resources_table.py rivulus_amd/csrc/build/resources.txt > out.txt
(two such tables, of two commits, diff line by line)"""
import hashlib
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
recs, cur = [], None
for line in open(sys.argv[1]):
    m = re.search(r"remark: Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}
        recs.append(cur)
        continue
    m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
    if m and cur is not None and m.group(1).strip() in FIELDS:
        cur[m.group(1).strip()] = m.group(2)
names = sorted({r["name"] for r in recs})
dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
dem = dict(zip(names, dem))
table = {}
for r in recs:
    table.setdefault(dem[r["name"]], set()).add(tuple(r.get(f, "?") for f in FIELDS))
print("# kernel | " + " ".join(f.split(" [")[0].replace(" ", "") for f in FIELDS) + " | copies (units the kernel is compiled into)")
copies = {}
for r in recs:
    copies[dem[r["name"]]] = copies.get(dem[r["name"]], 0) + 1
for k in sorted(table):
    shown = k if len(k) <= 150 else k[:150] + "...#" + hashlib.sha1(k.encode()).hexdigest()[:10]
    for t in sorted(table[k]):
        print(f"{shown} | {' '.join(t)} | {copies[k]}")
