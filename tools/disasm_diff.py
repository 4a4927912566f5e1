"""Two builds of a unit's gfx950 code object compared function by function, by demangled name.
    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only --no-gpu-bundle-output -c -o DIR/<unit>.co <unit>.hip
    llvm-objdump -d --no-show-raw-insn --no-leading-addr DIR/<unit>.co > DIR/<unit>.s        (in both trees)
    python3 tools/disasm_diff.py PARENT_DIR NEW_DIR unit...
Comments and symbol annotations are dropped, and so is the literal of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64: the
pc-relative distance to a callee or a table moves whenever anything before it in the code object grows or shrinks.  RENAME maps the
parent's names of kernels that were renamed on purpose (here: the join's wrappers).  Exit status 1 when a function's instructions
differ."""
import re
import subprocess
import sys

RENAME = [  # parent demangled name -> new demangled name
    (r"rvk::join_probe_count\(rvk::JoinProbeParams\)", "void rvk::join_probe_count<0>(rvk::JoinProbeParams, unsigned int*)"),
    (r"void rvk::join_probe_count_kind<(\d)>\(", r"void rvk::join_probe_count<\1>("),
    (r"void rvk::join_probe_count_batched<(\w+)>\(", r"void rvk::join_probe_count_batched<\1, 0>("),
    (r"void rvk::join_probe_count_batched_kind<", r"void rvk::join_probe_count_batched<"),
    (r"void rvk::join_probe_emit<(\d)>\(", r"void rvk::join_probe_emit<\1, 0>("),
    (r"void rvk::join_probe_emit_kind<", r"void rvk::join_probe_emit<"),
]


def functions(path):
    out, name, body, pc_relative = {}, None, [], 0
    for line in open(path):
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            if name:
                out[name] = body
            name, body = m.group(1), []
        elif name and line.strip():
            t = re.sub(r"\s*//.*$", "", line.strip())
            t = re.sub(r"\s*<[^>]*>", "", t)
            if pc_relative and re.match(r"s_addc?_u32 ", t):
                t = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pc-relative>", t)
                pc_relative -= 1
            else:
                pc_relative = 2 if t.startswith("s_getpc_b64") else 0
            body.append(t)
    if name:
        out[name] = body
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d: out[n] for n, d in zip(names, dem)}


def main():
    pdir, ndir, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    for u in units:
        old, new = functions(f"{pdir}/{u}.s"), functions(f"{ndir}/{u}.s")
        renamed = {}
        for k, v in old.items():
            nk = k
            for a, b in RENAME:
                nk2 = re.sub(a, b, nk)
                if nk2 != nk:
                    nk = nk2
                    break
            renamed[nk] = (k, v)
        same = differ = 0
        gone, added = [], []
        for k, (ok, v) in renamed.items():
            if k not in new:
                gone.append(ok)
            elif new[k] == v:
                same += 1
            else:
                differ += 1
                bad += 1
                print(f"  DIFFERS {u}: {ok} ({len(v)} -> {len(new[k])} instructions)")
        for k in new:
            if k not in renamed:
                added.append(k)
        print(f"{u}: {same} functions identical, {differ} differ, {len(gone)} only in parent, {len(added)} only in new")
        for g in gone:
            print(f"    only in parent: {g}")
        for g in added:
            print(f"    only in new: {g}")
    sys.exit(1 if bad else 0)


main()
