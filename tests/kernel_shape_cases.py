"""The enumeration of synthesis kernel shapes that tests/test_kernel_shapes.py pins and tests/tools/lds_sizes.py prints:

    precision {f64, mixed, f32} x SectionDelay {1, 2, 3, 4} x output rate {44100, 22050} x rows {1, 2, 4, 8}
    on the 10 + 6 tube, the same with SectionDelay 1 on the 30 + 18 tube (the 48-lane layout), and model 5 rows {1, 2}"""
import os

import gama_tts_amd as g
import oracle
from gama_tts_amd import capi

GOLDEN = os.path.join(oracle.GOLDEN_DIR, "kernel_shapes.json")
PRECISIONS = (("f64", capi.PRECISION_F64), ("mixed", capi.PRECISION_MIXED), ("f32", capi.PRECISION_F32))
ROWS = (1, 2, 4, 8)


def plans():
    """(name, config, is_model5) of every plan of the enumeration, in a fixed order."""
    cfgd = g.read_config_file(oracle.VOICE_MALE)
    for pname, prec in PRECISIONS:
        for layout, delays in ((capi.TUBE_10_6, (1, 2, 3, 4)), (capi.TUBE_30_18, (1,))):
            for delay in delays:
                for rate in (44100, 22050):
                    yield ("%s delay %d rate %d layout %d" % (pname, delay, rate, layout), g.config_from_dict(cfgd, float(rate), delay, prec, layout), False)
    yield ("model5", g.config5_from_dict(g.read_config_file(oracle.VOICE5_MALE)), True)


def launched_rows(name, rows):
    """The rows of the shape a launch with `rows` forced has (tests/test_kernel_shapes.py's docstring)."""
    if rows == 8 and (not name.startswith("f32") or name.endswith("layout 1")):
        return 4
    return rows


def lds_bytes():
    """{(plan name, rows): bytes} of every case, as the diagnostics library answers."""
    lib = g.load_library(diagnostics=True)
    out = {}
    for name, config, model5 in plans():
        plan = g.Plan(config, 250.0, capi.DEVICE_NONE, diagnostics=True)
        for rows in ((1, 2) if model5 else ROWS):
            out[name, rows] = int(lib.gvtm_debug_lds_bytes(plan._h, rows))
        plan.close()
    return out
