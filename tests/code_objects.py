"""The gfx950 code object inside a built file (an object file of csrc/_obj/, or a library), taken out with the LLVM binary
tools: what tests/test_codegen_signature.py reads its table from and tools/codeobj_diff.py compares two builds by.  A plain
module: no test, no fixture."""
import os
import re
import subprocess

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
# what a kernel's descriptor says of its registers, scratch bytes and LDS (llvm-readelf --notes: amdhsa.kernels)
DESCRIPTOR_KEYS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                   "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


def tool(name):
    return os.path.join(LLVM, name)


def tools_present():
    return all(os.path.exists(tool(t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"))


def unbundle(path, workdir):
    """The gfx950 code object of `path` as a file in `workdir`; None where `path` holds no device code."""
    fat, co = os.path.join(workdir, "fat.bin"), os.path.join(workdir, "k.co")
    subprocess.run([tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, fat], check=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.run([tool("clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    return co


def kernel_notes(co):
    """[(kernel name, its block of the code object's metadata)] in the metadata's order."""
    notes = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = []
    for block in re.split(r"(?=- \.agpr_count:)", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out.append((name.group(1), block))
    return out


def descriptor(block, keys=DESCRIPTOR_KEYS):
    return {key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1)) for key in keys}


def functions(co):
    """[(symbol, [instruction lines])] of the code object's text in symbol (address) order.  An instruction line is the
    opcode and its operands as llvm-objdump -d prints them: no address, no encoding; a branch target is a label, numbered
    by first appearance inside its function, and the label lines stay in the stream."""
    text = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", "--symbolize-operands", co],
                          check=True, capture_output=True, text=True).stdout
    out, labels = [], {}
    for line in text.splitlines():
        line = line.split("//")[0].rstrip()
        head = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if head and not re.fullmatch(r"L\d+", head.group(1)):
            out.append((head.group(1), []))
            labels = {}
        elif out and line.strip():
            relabel = lambda m: "L%d" % labels.setdefault(m.group(0), len(labels))  # noqa: E731
            out[-1][1].append(re.sub(r"\bL\d+\b", relabel, " ".join(line.split())))
    return out
