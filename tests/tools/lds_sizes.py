"""LDS bytes per workgroup of every kernel shape (runs without a GPU; diagnostics library): the enumeration
of tests/kernel_shape_cases.py (pinned by tests/test_kernel_shapes.py), in KB."""
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import kernel_shape_cases as shapes  # noqa: E402

by_plan = {}
for (name, rows), lds in shapes.lds_bytes().items():
    by_plan.setdefault(name, []).append((rows, lds))
for name, sizes in by_plan.items():
    print(name, "KB for", "/".join(str(r) for r, _ in sizes), "utterances per workgroup:", [round(b / 1024, 1) for _, b in sizes])
