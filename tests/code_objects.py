"""The gfx950 code object of a built kernel file, as the host tests read it: the kernels of protoquant_amd/csrc/build/<objname>.o with the notes that say whether one
uses scratch or spills (as `make spillcheck` reads the GEMM objects), and the disassembly of the whole code object when asked for.  Needs no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE = re.compile(r"\.(name|private_segment_fixed_size|sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count):\s+(\S+)")


def kernels_of(objname, disassembly=False, must_be_built=False):
    """{mangled kernel name: {note: value}} of build/<objname>.o (with disassembly: that and the llvm-objdump listing).  Skips where the ROCm LLVM tools are missing
    and where the object was not built; must_be_built makes the latter a failure instead."""
    obj = os.path.join(ROOT, "protoquant_amd", "csrc", "build", objname + ".o")
    llvm = os.environ.get("LLVMBIN", "/opt/rocm/lib/llvm/bin")
    if must_be_built:
        if not os.path.exists(os.path.join(llvm, "llvm-readelf")):
            pytest.skip("needs the ROCm LLVM tools")
        assert os.path.exists(obj), f"{obj} was not built"
    elif not os.path.exists(obj) or not os.path.exists(os.path.join(llvm, "llvm-readelf")):
        pytest.skip("needs the built object and the ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, objname + ".fatbin"), os.path.join(tmp, objname + ".co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "unused.o")], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                       check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout if disassembly else None
    kernels, name = {}, None
    for ln in notes.splitlines():
        m = NOTE.search(ln)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return (kernels, dis) if disassembly else kernels
