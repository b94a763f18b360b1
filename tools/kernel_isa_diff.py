"""Compares the device code of two builds function by function: the instruction text and the resource figures.

    hipcc --offload-arch=gfx950 <product flags> --cuda-device-only -S csrc/X.hip -o X.s     (one listing per .hip file)
    python tools/kernel_isa_diff.py before/*.s -- after/*.s [--resources table.txt]

A listing is cut at its function symbols; comments, .loc / .file and alignment directives are dropped and the numbers of the
local labels (.LBB<n>_, .LJTI<n>_) normalised, since they count the functions of a file.  Every function of the `after`
listings must exist in `before` with the same text, .amdhsa_ lines and register / scratch / LDS / occupancy figures, and no
function of `before` may be missing (a function that several files hold, such as a __noinline__ one, is compared once per
copy).  --resources writes the after side's figures as a table.  Exit status 1 on any difference.
"""
import re
import subprocess
import sys

STATS = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")


def functions(path):
    """{symbol: (text lines, resource lines)} for every function of a listing"""
    out, name, text, res, in_body = {}, None, [], [], False
    for raw in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if m:
            name, text, res, in_body = m.group(1), [], [], True
            out[name] = (text, res)
            continue
        if ".amdgpu_metadata" in raw:
            name = None
        if name is None:
            continue
        s = re.match(r"\s*;\s*(\w+):\s*(\S+)", raw)
        if s and s.group(1) in STATS and not in_body:
            res.append(f"{s.group(1)} {s.group(2)}")
            continue
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            in_body = False
            continue
        if line.startswith(".amdhsa_") and not line.startswith(".amdhsa_kernel"):
            res.append(line)
            continue
        if not in_body or re.match(r"\.(loc|file|p2align|align|section|text|size|end_amdhsa_kernel|amdhsa_kernel|cfi_)\b", line):
            continue
        text.append(re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", line))
    return out


def short(sym):
    dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*", "", dem).replace("void mcrt::", "").replace("mcrt::", "")


def main(argv):
    table = None
    if "--resources" in argv:
        i = argv.index("--resources")
        table, argv = argv[i + 1], argv[:i] + argv[i + 2:]
    cut = argv.index("--")
    before = {}
    for p in argv[:cut]:
        before.update(functions(p))
    bad, seen, rows = 0, set(), []
    for p in argv[cut + 1:]:
        for sym, (text, res) in functions(p).items():
            seen.add(sym)
            fig = dict(r.split(" ", 1) for r in res if r.split(" ", 1)[0] in STATS)
            rows.append(f"{short(sym):42s} vgpr {fig.get('NumVgprs', '?'):>4s} agpr {fig.get('NumAgprs', '?'):>3s} sgpr {fig.get('TotalNumSgprs', '?'):>4s} "
                        f"scratch {fig.get('ScratchSize', '?'):>4s} occ {fig.get('Occupancy', '?'):>2s} lds {fig.get('LDSByteSize', '?'):>6s}  ({p.rsplit('/', 1)[-1]})")
            if sym not in before:
                print(f"NEW        {short(sym)}  ({p})")
                bad += 1
                continue
            t0, r0 = before[sym]
            same_text, same_res = t0 == text, r0 == res
            print(f"{'same' if same_text and same_res else 'DIFFERENT':10s} {len(text):6d} lines  {short(sym)}")
            if not same_text:
                first = next((i for i, (a, b) in enumerate(zip(t0, text)) if a != b), min(len(t0), len(text)))
                print(f"           text: {len(t0)} -> {len(text)} lines, first difference at line {first}")
            if not same_res:
                print("           resources: " + "; ".join(f"{a} -> {b}" for a, b in zip(r0, res) if a != b))
            bad += not (same_text and same_res)
    for sym in before:
        if sym not in seen:
            print(f"MISSING    {short(sym)}")
            bad += 1
    print(f"{len(seen)} functions of {len(before)} compared, {bad} difference(s)")
    if table:
        open(table, "w").write("\n".join(rows) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
