#!/usr/bin/env python3
"""Compare the gfx950 kernels of two built csrc/build directories, object by object and kernel by kernel (the table of profiles/r17_rownorm_kernels.txt).

    python tools/kernel_identity.py PARENT/protoquant_amd/csrc/build protoquant_amd/csrc/build [--map REGEX=REPL ...] [--objects REGEX] [--diff REGEX] [-o profiles/NAME.txt]

Per object: the sha256 of the unbundled code object; where it differs, per kernel: instruction-identical or not, and VGPRs, SGPRs, scratch bytes, spills and waves
per SIMD of both sides.  Needs no GPU: it unbundles each object (llvm-objcopy, clang-offload-bundler), reads the notes (llvm-readelf) and compares the disassembly
(llvm-objdump) as instruction lists.
Method.  The listing is cut per kernel symbol; addresses, encodings and the padding after the last s_endpgm are dropped, and the immediate offset of every
s_load_dword* is masked (they load from the kernarg pointer: a kernel that takes another argument list has other offsets and is otherwise the same program).
"identical" = the two lists are then equal line for line, registers included.  waves/SIMD = min(8, floor(512 / (ceil(vgpr / 8) * 8))).
Kernels are paired by demangled name (llvm-cxxfilt or c++filt) without the argument list; --map rewrites the PARENT's names first (re.sub, applied in order), for a
kernel that was renamed:
    --map '^pq::gemma_rmsnorm_quant_rows<(.*)>$=pq::rmsnorm_quant_rows<\\1, pq::GemmaGain, true>'
--objects compares only the object files whose name matches (a quick look at one object while trying variants); --diff prints the instruction diff of the kernels
that are not identical and whose name matches."""
import argparse
import difflib
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVMBIN", "/opt/rocm/lib/llvm/bin")
NOTE = re.compile(r"\.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """the gfx950 code object of a host object file, or None when it carries no device code"""
    fat, co = os.path.join(tmp, "o.fatbin"), os.path.join(tmp, "o.co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "unused.o")], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return None
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return co if os.path.getsize(co) else None


def kernels_of(co):
    """{demangled name without arguments: (notes, instruction list)}"""
    meta, name = {}, None
    for ln in tool("llvm-readelf", "--notes", co).splitlines():
        m = NOTE.search(ln)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    body, cur = {}, None
    for ln in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", ln)
        if m:
            cur = body.setdefault(m.group(1), []) if m.group(1) in meta else None
        elif cur is not None and ln.strip():
            ins = re.sub(r"\s+", " ", ln.split("//")[0]).strip()
            cur.append(re.sub(r"^(s_load_dword\w* .*), \S+$", r"\1, <kernarg>", ins))
    for ins in body.values():
        while ins and not ins[-1].startswith("s_endpgm"):
            ins.pop()
    names = list(meta)
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    plain = subprocess.run([filt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines() if names and filt else names
    out = {}
    for n, d in zip(names, plain):
        key = re.sub(r"^void ", "", d)
        depth, end = 0, len(key)
        for i, c in enumerate(key):          # cut the argument list: the first '(' outside the template arguments
            depth += c == "<"
            depth -= c == ">"
            if c == "(" and depth == 0:
                end = i
                break
        out[key[:end]] = (meta[n], body.get(n, []))
    return out


def waves(vgpr):
    return min(8, 512 // (-(-vgpr // 8) * 8)) if vgpr else 8


def facts(m):
    return "vgpr %3d sgpr %3d scratch %d spills %d waves %d" % (m.get("vgpr_count", 0), m.get("sgpr_count", 0), m.get("private_segment_fixed_size", 0),
                                                                m.get("vgpr_spill_count", 0) + m.get("sgpr_spill_count", 0), waves(m.get("vgpr_count", 0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL", help="rewrite the parent's kernel names before pairing")
    ap.add_argument("--objects", metavar="REGEX", help="compare only the objects whose file name matches")
    ap.add_argument("--diff", metavar="REGEX", help="print the instruction diff of every kernel that is not identical and whose name matches")
    ap.add_argument("-o", "--output")
    a = ap.parse_args()
    maps = [m.split("=", 1) for m in a.map]
    out = open(a.output, "w") if a.output else sys.stdout
    objs = sorted({f for d in (a.parent, a.new) for f in os.listdir(d) if f.endswith(".o") and not f.startswith(".") and re.search(a.objects or "", f)})
    total = same = 0
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tn:
        for o in objs:
            po, no = os.path.join(a.parent, o), os.path.join(a.new, o)
            if not (os.path.exists(po) and os.path.exists(no)):
                print(f"{o}: only in the {'parent' if os.path.exists(po) else 'new'} build", file=out)
                continue
            pc, nc = code_object(po, tp), code_object(no, tn)
            if pc is None or nc is None:
                print(f"{o}: no gfx950 code object", file=out)
                continue
            ph, nh = (hashlib.sha256(open(c, "rb").read()).hexdigest()[:16] for c in (pc, nc))
            if ph == nh:
                print(f"{o}: code object sha256 equal {ph}", file=out)
                continue
            pk, nk = kernels_of(pc), kernels_of(nc)
            renamed = {}
            for k, v in pk.items():
                for rx, repl in maps:
                    k = re.sub(rx, repl, k)
                renamed[k] = v
            ident = [k for k in nk if k in renamed and renamed[k][1] == nk[k][1]]
            total += len(nk)
            same += len(ident)
            print(f"{o}: code object sha256 {ph} -> {nh}; {len(pk)} -> {len(nk)} kernels, {len(ident)} instruction-identical", file=out)
            for k in sorted(nk):
                if k not in renamed:
                    print(f"    NEW        {k}: {facts(nk[k][0])}", file=out)
                elif k in ident:
                    pm, nm = renamed[k][0], nk[k][0]
                    print(f"    identical  {k}: {facts(nm)}" + ("" if facts(pm) == facts(nm) else f"   (parent: {facts(pm)})"), file=out)
                else:
                    print(f"    DIFFERENT  {k}: {facts(renamed[k][0])} ({len(renamed[k][1])} instructions) -> {facts(nk[k][0])} ({len(nk[k][1])})", file=out)
                    if a.diff and re.search(a.diff, k):
                        print("\n".join(difflib.unified_diff(renamed[k][1], nk[k][1], "parent", "new", n=2, lineterm="")), file=out)
            for k in sorted(set(renamed) - set(nk)):
                print(f"    GONE       {k}: {facts(renamed[k][0])}", file=out)
    print(f"kernels of the objects that changed: {total}, instruction-identical to the parent's: {same}", file=out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
