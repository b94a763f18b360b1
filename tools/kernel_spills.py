"""Per-kernel scalar-register spills of the device code: what the compiler reports, and the lane moves it emitted for them.

    python tools/kernel_spills.py [libmcrt.so | file.hip] [--all]      (default: the package's built library)

A library: its gfx950 code objects are cut out of the offload bundles it embeds.  A source file: compiled for the device
alone with the product's flags (minecraftskin_raytracer_amd/build.py).  Per kernel one line: SGPRs, .sgpr_spill_count,
VGPRs, .vgpr_spill_count, scratch bytes per lane (the kernel's metadata note), then the static count of lane read-backs
(v_readlane_b32) and write-outs (v_writelane_b32) in its code and how many of each lie inside a loop — between a backward
branch and its target.  Without --all only the kernels of the render pipeline's hot path are printed.

An SGPR the register allocator could not keep is parked in a VGPR lane by a write-out and fetched by a read-back; both
are VALU instructions ("Scalar registers").  The tool reads compiler output only: the metadata note and the
disassembly's two lane-move mnemonics and branches.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
ARCH = "gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
HOT = ("primary_kernel", "primary_batch_kernel", "lit_kernel", "lit_batch_kernel", "resolve_kernel", "resolve_batch_kernel",
       "resolve_transparent_kernel", "resolve_transparent_batch_kernel", "ao_kernel", "ao_batch_kernel", "plan_tiles_kernel")


def code_objects(path):
    """the gfx950 ELF images embedded in a host library (one per .hip source)"""
    blob = open(path, "rb").read()
    if blob[:4] == b"\x7fELF" and struct.unpack_from("<H", blob, 18)[0] == 224:  # a bare AMDGPU code object
        return [blob]
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if ARCH in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + len(MAGIC))
    return out


def compile_device(src, tmp):
    sys.path.insert(0, ROOT)
    from minecraftskin_raytracer_amd import build as B

    out = os.path.join(tmp, "device.co")
    subprocess.check_call([B._hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", f"-I{os.path.join(ROOT, 'include')}",
                           f"-I{B.CSRC}", *os.environ.get("MCRT_EXTRA_FLAGS", "").split(), "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", out])
    return open(out, "rb").read()


def metadata(elf_path):
    """{kernel symbol: {field: int}} from the code object's metadata note"""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf_path], capture_output=True, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"(  - |    )\.(\w+):\s*(.*)$", line)  # a kernel's own fields; its arguments' sit deeper
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        key, val = m.group(2), m.group(3).strip().strip("'")
        if cur is None:
            continue
        if key == "name":
            kernels[val] = cur
        elif re.fullmatch(r"-?\d+", val):
            cur[key] = int(val)
    return kernels


def lane_moves(elf_path):
    """{symbol: (read-backs, write-outs, read-backs in loops, write-outs in loops)} from the disassembly"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f"--mcpu={ARCH}", elf_path], capture_output=True, text=True, check=True).stdout
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-fA-F]+ <(\S+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        m = re.match(r"\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    out = {}
    for sym, ins in funcs.items():
        loops = []
        for addr, op, args in ins:
            if op.startswith(("s_branch", "s_cbranch")) and re.fullmatch(r"\d+", args):
                imm = int(args)
                imm -= 0x10000 if imm >= 0x8000 else 0
                target = addr + 4 + 4 * imm
                if target <= addr:
                    loops.append((target, addr))
        inside = lambda a: any(lo <= a <= hi for lo, hi in loops)
        rd = [a for a, op, _ in ins if op == "v_readlane_b32"]
        wr = [a for a, op, _ in ins if op == "v_writelane_b32"]
        out[sym] = (len(rd), len(wr), sum(map(inside, rd)), sum(map(inside, wr)))
    return out


def short(sym):
    dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*", "", dem).replace("void mcrt::", "").replace("mcrt::", "")


def kernel_rows(path):
    """[(short name, {sgpr, sgpr_spill, vgpr, vgpr_spill, scratch, read, write, read_loop, write_loop})] for a library or a source file"""
    rows = []
    with tempfile.TemporaryDirectory(prefix="mcrt_spills_") as tmp:
        images = code_objects(path) if not path.endswith((".hip", ".cpp")) else [compile_device(path, tmp)]
        if not images:
            raise SystemExit(f"{path}: no {ARCH} code object found")
        for i, image in enumerate(images):
            elf = os.path.join(tmp, f"image{i}.co")
            open(elf, "wb").write(image)
            moves = lane_moves(elf)
            for sym, md in metadata(elf).items():
                rd, wr, rdl, wrl = moves.get(sym, (0, 0, 0, 0))
                rows.append((short(sym), dict(sgpr=md.get("sgpr_count", -1), sgpr_spill=md.get("sgpr_spill_count", 0), vgpr=md.get("vgpr_count", -1),
                                              vgpr_spill=md.get("vgpr_spill_count", 0), scratch=md.get("private_segment_fixed_size", 0),
                                              kernarg=md.get("kernarg_segment_size", 0), read=rd, write=wr, read_loop=rdl, write_loop=wrl)))
    return sorted(rows)


def main(argv):
    show_all = "--all" in argv
    args = [a for a in argv if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "minecraftskin_raytracer_amd", "libmcrt.so")
    print(f"{'kernel':44s} kernarg sgpr sgpr_spill vgpr vgpr_spill scratch  readlane (in loops)  writelane (in loops)")
    for name, r in kernel_rows(path):
        if not show_all and re.sub(r"<.*", "", name) not in HOT:
            continue
        print(f"{name:44s} {r['kernarg']:7d} {r['sgpr']:4d} {r['sgpr_spill']:10d} {r['vgpr']:4d} {r['vgpr_spill']:10d} {r['scratch']:7d}  "
              f"{r['read']:8d} ({r['read_loop']:8d})  {r['write']:9d} ({r['write_loop']:8d})")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
