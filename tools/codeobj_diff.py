#!/usr/bin/env python3
"""usage: codeobj_diff.py A B     (two object files, or two directories of them such as gama_tts_amd/csrc/_obj)

Compares the gfx950 code objects of two builds, unit by unit: the kernels each holds in symbol order and, per kernel, the
opcode-and-operand stream of the disassembly (no addresses, no encodings, branch targets as labels; tests/code_objects.py)
and the descriptor's registers, scratch bytes and LDS.  One line per unit: "n kernels identical, same order", or what
differs.  A literal that moves with the layout (a pc-relative address) is compared as it stands: a kernel whose only
differences are literals is named as such, and still counts as a difference.  Exit status 1 when anything differs.

This is the check behind "disassembles to the parent's instructions": build the parent in a scratch worktree, then
    tools/codeobj_diff.py <parent>/gama_tts_amd/csrc/_obj gama_tts_amd/csrc/_obj"""
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import code_objects  # noqa: E402


def read(path):
    """(kernel names in symbol order, {symbol: instruction lines}, {kernel: descriptor}) of a file; None: no device code."""
    with tempfile.TemporaryDirectory() as wd:
        co = code_objects.unbundle(path, wd)
        if co is None:
            return None
        descriptors = {name: code_objects.descriptor(block) for name, block in code_objects.kernel_notes(co)}
        functions = code_objects.functions(co)
    return [name for name, _ in functions if name in descriptors], dict(functions), descriptors


def compare(a, b):
    """The differences of two files, as words; empty: none.  Second value: the number of kernels."""
    a, b = read(a), read(b)
    if a is None or b is None:
        return ([] if a is b else ["only one side holds device code"]), 0
    (order_a, code_a, desc_a), (order_b, code_b, desc_b) = a, b
    said = ["only in A: " + n for n in order_a if n not in desc_b] + ["only in B: " + n for n in order_b if n not in desc_a]
    if not said and order_a != order_b:
        said.append("the same kernels in another order")
    if sorted(code_a) != sorted(code_b):
        said.append("other device functions: " + " ".join(sorted(set(code_a) ^ set(code_b))))
    for name in sorted(set(code_a) & set(code_b)):
        what = []
        if code_a[name] != code_b[name]:
            masked = [[re.sub(r"\b0x[0-9a-f]+\b", "0x", line) for line in code[name]] for code in (code_a, code_b)]
            what.append("literals" if masked[0] == masked[1] else "instructions (%d against %d)" % (len(code_a[name]), len(code_b[name])))
        if name in desc_a and name in desc_b and desc_a[name] != desc_b[name]:
            what.append("descriptor " + " ".join("%s %d -> %d" % (k, v, desc_b[name][k]) for k, v in desc_a[name].items() if v != desc_b[name][k]))
        if what:
            said.append("%s: %s" % (name, ", ".join(what)))
    return said, len(order_a)


def main(a, b):
    if os.path.isdir(a) != os.path.isdir(b):
        sys.exit("A and B: two files or two directories")
    if os.path.isdir(a):
        names = sorted(n for n in set(os.listdir(a)) | set(os.listdir(b)) if n.endswith(".o"))
        pairs = [(n, os.path.join(a, n), os.path.join(b, n)) for n in names]
    else:
        pairs = [(os.path.basename(a) if os.path.basename(a) == os.path.basename(b) else a + " " + b, a, b)]
    differ = False
    for unit, pa, pb in pairs:
        if not os.path.exists(pa) or not os.path.exists(pb):
            said, n = ["only in " + ("B" if os.path.exists(pb) else "A")], 0
        else:
            said, n = compare(pa, pb)
        differ = differ or bool(said)
        print("%-34s %s" % (unit, "; ".join(said) if said else ("%d kernels identical, same order" % n if n else "no device code")))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
