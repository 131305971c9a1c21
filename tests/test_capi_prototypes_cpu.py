"""gama_tts_amd/capi.py against the C it binds: the two prototype tables against the declarations of include/gama_vtm.h and
the definitions of csrc/vtm_capi_hooks.cpp, and the ctypes structures, numpy record layouts and constants against what a C
compiler makes of the header.  Almost every parameter is a pointer or a size_t, so a wrong argtypes list would not crash:
it would hand the device a truncated or shifted value.

Known limit: the check is by type, so it cannot see two parameters of one type swapped.  One entry invites that:
gvtm_synthesize_voices_device (and its two host forms) takes max_frames BEFORE batch, unlike every sibling.  The order in
which the wrappers pass their arguments is what the GPU tests cover (test_gpu_voices.py and the other callers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gama_tts_amd as g
from gama_tts_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gama_vtm.h")
HOOKS = os.path.join(ROOT, "gama_tts_amd", "csrc", "vtm_capi_hooks.cpp")
STRUCTS = {"gvtm_config": capi.Config, "gvtm5_config": capi.Config5, "gvtm_info": capi.Info, "gvtm_track_config": capi.TrackConfig,
           "gvtm_packed_stats": capi.PackedStats}
RECORDS = {"gvtm_event": capi.EVENT_DTYPE, "gvtm_drift_state": capi.DRIFT_DTYPE, "gvtm_intonation_point": capi.POINT_DTYPE}
SCALARS = {"int": "int", "int32_t": "int", "size_t": "size_t", "int64_t": "int64_t", "double": "double", "void": "void"}
CTYPES = {ctypes.c_int: "int", ctypes.c_size_t: "size_t", ctypes.c_int64: "int64_t", ctypes.c_double: "double",
          ctypes.c_char_p: "const char*", None: "void"}


def read(path):
    with open(path) as f:
        return f.read()


def strip_comments(text):
    """C text without its comments, its string literals emptied (one pass, so neither is looked for inside the other) and
    its preprocessor lines dropped."""
    text = re.sub(r'"(?:\\.|[^"\\\n])*"|/\*.*?\*/|//[^\n]*', lambda m: '""' if m.group().startswith('"') else " ", text, flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)


def c_class(text, parameter):
    """A C return type or parameter declaration -> (class, pointee): class one of pointer, size_t, int, int64_t, double,
    const char*, void; pointee the type a pointer points to (None for an array parameter)."""
    text = " ".join(text.replace("*", " * ").split())
    if "[" in text:
        return "pointer", None
    if "*" in text:
        pointee = " ".join(w for w in text[: text.index("*")].split() if w != "const")
        return ("const char*", None) if pointee == "char" else ("pointer", pointee)
    words = [w for w in text.split() if w != "const"]
    if parameter and len(words) > 1:
        words = words[:-1]  # its name
    return SCALARS.get(" ".join(words), "unknown type '%s'" % text), None


def c_prototypes(text, definitions=False):
    """name -> (return class, [parameter classes]) of every gvtm_* function that C text declares (`...);`) or, with
    definitions, defines (`...) {`) at the start of a line; a declaration may run over several lines."""
    found = {}
    for ret, name, params, end in re.findall(r"^([A-Za-z_][\w \t\*]*?)\b(gvtm_\w+)\s*\(([^()]*)\)\s*([;{])", strip_comments(text), flags=re.M):
        if end == ("{" if definitions else ";"):
            params = [p for p in params.split(",") if p.strip() not in ("", "void")]
            found[name] = (c_class(ret, False), [c_class(p, True) for p in params])
    return found


def table_class(ctype):
    if ctype is ctypes.c_void_p:
        return "pointer", None
    if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
        return "pointer", ctype._type_
    return CTYPES.get(ctype, "unknown ctype %r" % (ctype,)), None


def agree(c, table):
    """A C class against a table entry's: equal classes, and a pointer to one of the binding's structures is typed as that
    structure, any other pointer is a plain c_void_p."""
    (c_kind, pointee), (t_kind, structure) = c, table
    return c_kind == t_kind and structure is STRUCTS.get(pointee)


def problems(declared, table):
    """Every disagreement between C prototypes and a prototype table, each one naming its function."""
    out = ["%s: declared in C, not in the table" % n for n in declared if n not in table]
    out += ["%s: in the table, not declared in C" % n for n in table if n not in declared]
    for name in declared:
        if name not in table:
            continue
        (ret, params), (restype, argtypes) = declared[name], table[name]
        if not agree(ret, table_class(restype)):
            out.append("%s: returns %s, the table says %r" % (name, ret[0], restype))
        if len(params) != len(argtypes):
            out.append("%s: %d parameters, the table has %d" % (name, len(params), len(argtypes)))
            continue
        out += ["%s: parameter %d is %s, the table says %r" % (name, k, p, a) for k, (p, a) in enumerate(zip(params, argtypes))
                if not agree(p, table_class(a))]
    return out


def test_tables_agree_with_the_header_and_the_hooks_file():
    header, hooks = c_prototypes(read(HEADER)), c_prototypes(read(HOOKS), definitions=True)
    assert len(header) >= 60 and "gvtm_synthesize_intonation_device" in header and "gvtm_last_error" in header, sorted(header)
    assert len(hooks) >= 18 and "gvtm_debug_tracks_slice" in hooks and all(n.startswith("gvtm_debug_") for n in hooks), sorted(hooks)
    assert not any(n.startswith("gvtm_debug_") for n in header)
    assert header["gvtm_plan_table"] == (("int", None), [("pointer", "gvtm_plan"), ("int", None), ("pointer", "double"), ("size_t", None)])
    assert header["gvtm_last_error"] == (("const char*", None), [])
    assert hooks["gvtm_debug_launch_shape"][1][3] == ("pointer", None)  # size_t out[3]
    assert problems(header, capi.PROTOTYPES) == []
    assert problems(hooks, capi.HOOK_PROTOTYPES) == []
    assert set(capi._REQUIRED) <= set(capi.PROTOTYPES)


def _doctor(old, new):
    def edit(text):
        assert text.count(old) == 1, old
        return text.replace(old, new)
    return edit


@pytest.mark.parametrize("name,edit,says", [
    ("gvtm_plan_table", _doctor("double* out, size_t capacity);", "double* out);"), "3 parameters, the table has 4"),
    ("gvtm_output_count", _doctor("size_t gvtm_output_count(const gvtm_plan* plan, size_t n_frames);",
                                  "size_t gvtm_output_count(const gvtm_plan* plan, int n_frames);"), "parameter 1 is ('int', None)"),
    ("gvtm_plan_reserve", _doctor("int gvtm_plan_reserve(", "size_t gvtm_plan_reserve("), "returns size_t"),
    ("gvtm_plan_reserve", _doctor("int gvtm_plan_reserve(gvtm_plan* plan, size_t max_frames);", ""), "in the table, not declared in C"),
    ("gvtm_plan_shrink", lambda text: text + "\nint gvtm_plan_shrink(gvtm_plan* plan,\n\t\tsize_t max_frames);\n", "declared in C, not in the table"),
    ("gvtm_plan_create_model5", _doctor("int gvtm_plan_create_model5(const gvtm5_config* config", "int gvtm_plan_create_model5(const gvtm_config* config"),
     "parameter 0 is ('pointer', 'gvtm_config')"),
    ("gvtm_stream_get_drift", _doctor("gvtm_drift_state* states_out /* [batch], host */);", "gvtm_info* states_out /* [batch], host */);"),
     "parameter 1 is ('pointer', 'gvtm_info')"),
], ids=["parameter-dropped", "size_t-to-int", "int-return-to-size_t", "function-removed", "function-added", "other-structure", "structure-for-plain"])
def test_the_checker_reports_a_doctored_header(name, edit, says):
    found = problems(c_prototypes(edit(read(HEADER))), capi.PROTOTYPES)
    assert len(found) == 1 and found[0].startswith(name + ": ") and says in found[0], found


def test_the_checker_reports_a_doctored_hooks_file_and_a_doctored_table():
    edit = _doctor("int gvtm_debug_chunk_length(const gvtm_plan* plan, size_t batch)", "int gvtm_debug_chunk_length(const gvtm_plan* plan, int batch)")
    hooks = c_prototypes(edit(read(HOOKS)), True)
    found = problems(hooks, capi.HOOK_PROTOTYPES)
    assert len(found) == 1 and found[0].startswith("gvtm_debug_chunk_length: parameter 1 is ('int', None)"), found
    table = dict(capi.HOOK_PROTOTYPES, gvtm_debug_lds_bytes=(ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]))
    found = problems(c_prototypes(read(HOOKS), True), table)
    assert len(found) == 1 and found[0].startswith("gvtm_debug_lds_bytes: returns size_t"), found


@pytest.mark.parametrize("diagnostics", [False, True])
def test_a_loaded_library_carries_exactly_the_tables_types(diagnostics):
    lib = g.load_library(diagnostics)
    table = {**capi.PROTOTYPES, **capi.HOOK_PROTOTYPES} if diagnostics else capi.PROTOTYPES
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    if not diagnostics:  # the product library has none of the hooks, so the binding declares none on it
        exported = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
        assert "gvtm_plan_create" in exported and "gvtm_debug_" not in exported
        assert not any(hasattr(lib, name) for name in capi.HOOK_PROTOTYPES)


# ---- structures, record layouts and constants against the compiler's view of the header ----

KINDS = {"double": "f", "int32_t": "i", "uint32_t": "u", "size_t": "u"}
CONSTANTS = [("GVTM_N_PARAM", capi.N_PARAM), ("GVTM_PACKED_ALIGN", capi.PACKED_ALIGN), ("GVTM_MAX_INTONATION_POINTS", capi.MAX_INTONATION_POINTS),
             ("GVTM_DEVICE_NONE", capi.DEVICE_NONE), ("GVTM_PRECISION_F64", capi.PRECISION_F64), ("GVTM_PRECISION_MIXED", capi.PRECISION_MIXED),
             ("GVTM_PRECISION_F32", capi.PRECISION_F32), ("GVTM_TUBE_10_6", capi.TUBE_10_6), ("GVTM_TUBE_30_18", capi.TUBE_30_18),
             ("GVTM_TABLE_FIR", capi.TABLE_FIR), ("GVTM_TABLE_SRC_H", capi.TABLE_SRC_H), ("GVTM_TABLE_SRC_DH", capi.TABLE_SRC_DH),
             ("GVTM_TABLE_WAVETABLE", capi.TABLE_WAVETABLE), ("GVTM_ERR_UNSUPPORTED", capi._STATUS_UNSUPPORTED)]


def c_struct_fields(text):
    """struct name -> [(field, kind)] in order, kind f / i / u, of every `typedef struct NAME { ... } NAME;` with a body."""
    found = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", strip_comments(text)):
        fields = []
        for declaration in filter(None, (d.strip() for d in body.split(";"))):
            ctype, names = declaration.split(None, 1)
            fields += [(n.split("[")[0].strip(), KINDS[ctype]) for n in names.split(",")]
        found[name] = fields
    return found


@pytest.fixture(scope="module")
def c_view(tmp_path_factory):
    """(layouts, constants) as gcc sees include/gama_vtm.h in C99: layouts[struct] = (sizeof, [(field, kind, offsetof, size)]),
    the fields as the header lists them."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = c_struct_fields(read(HEADER))
    assert set(structs) == set(STRUCTS) | set(RECORDS), sorted(structs)
    lines = ["#include <stdio.h>", '#include "gama_vtm.h"',
             '#define FIELD(S, f) printf("field %s %s %zu %zu\\n", #S, #f, offsetof(S, f), sizeof(((S*)0)->f))', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('printf("struct %s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ["FIELD(%s, %s);" % (name, field) for field, _ in fields]
    lines += ['printf("constant %s %%d\\n", (int)(%s));' % (name, name) for name, _ in CONSTANTS]
    lines += ["return 0;", "}"]
    tmp = tmp_path_factory.mktemp("layout")
    (tmp / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(tmp / "layout.c"),
                    "-o", str(tmp / "layout")], check=True)
    layouts, constants = {}, {}
    for line in subprocess.run([str(tmp / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        what, name, *rest = line.split()
        if what == "struct":
            layouts[name] = (int(rest[0]), [])
        elif what == "field":
            kind = dict(structs[name])[rest[0]]
            layouts[name][1].append((rest[0], kind, int(rest[1]), int(rest[2])))
        else:
            constants[name] = int(rest[0])
    return layouts, constants


def ctypes_layout(structure):
    def kind(ctype):
        while issubclass(ctype, ctypes.Array):
            ctype = ctype._type_
        return {"d": "f", "f": "f"}.get(ctype._type_, "i" if ctype._type_.islower() else "u")  # struct-module codes: lower case is signed
    return ctypes.sizeof(structure), [(name, kind(ctype), getattr(structure, name).offset, getattr(structure, name).size)
                                      for name, ctype in structure._fields_]


def numpy_layout(dtype):
    return dtype.itemsize, [(name, dtype.fields[name][0].base.kind, dtype.fields[name][1], dtype.fields[name][0].itemsize) for name in dtype.names]


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_ctypes_structure_is_the_c_struct(c_view, name):
    assert ctypes_layout(STRUCTS[name]) == c_view[0][name]


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_numpy_record_layout_is_the_c_struct(c_view, name):
    assert numpy_layout(RECORDS[name]) == c_view[0][name]


def test_constants_are_the_headers(c_view):
    assert c_view[1] == dict(CONSTANTS)
    assert [c_view[0][name][0] for name in sorted(RECORDS)] == [40, 296, 24]  # the sizes the header's text and DESIGN.md quote


def test_the_layout_check_sees_a_moved_a_resized_and_a_widened_field(c_view):
    want = c_view[0]["gvtm_info"]
    fields = list(capi.Info._fields_)

    def doctored(new_fields):
        return ctypes_layout(type("Doctored", (ctypes.Structure,), {"_fields_": new_fields}))

    assert doctored(fields) == want
    assert doctored(fields[:4] + [fields[5], fields[4]] + fields[6:]) != want  # fir_taps and time_register_increment change places
    assert doctored([(n, ctypes.c_int64 if n == "pad_size" else t) for n, t in fields]) != want  # a 32-bit field declared as 64-bit
    assert doctored([(n, ctypes.c_uint32 if n == "pad_size" else t) for n, t in fields]) != want  # ... or as unsigned
    config = [(n, ctypes.c_double * 6 if n == "nasal_radius" else t) for n, t in capi.Config._fields_]
    assert doctored(config) != c_view[0]["gvtm_config"] == ctypes_layout(capi.Config)  # an array one element longer
    moved = np.dtype([("time_ms", "<i4"), ("has_interp", "<i4"), ("param", "<f8", 16), ("interp", "<f8", 4), ("special", "<f8", 16)])
    assert numpy_layout(moved) != c_view[0]["gvtm_event"]
