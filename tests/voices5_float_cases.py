"""Plans of several voices of the float class of reference model 5 (gvtm_plan_create_model5_float_voices): the five
5_male variants as float configurations, the plan of all of them (rows 1 / 2: a diagnostics plan forced to chunk 60 / 56),
the entry called by hand for the refusals, and every utterance of a mixed batch through the single-voice float plan of its
voice (gvtm_plan_create_model5_float), which a mixed launch has to reproduce bit for bit.  Shared by
test_capi_voices5_float_cpu.py and test_gpu_voices5_float.py."""
import ctypes

import numpy as np

import gama_tts_amd as g
from gama_tts_amd import capi
from parity_rules import TOL, within
from voice_files import VOICES, voice_path

BIT_IDENTICAL = TOL[capi.PRECISION_F32]


def configs5f(rate=48000.0, names=VOICES, overrides=None):
    """One float Config5 per name; overrides: {index: {key: value}} on that voice's file."""
    out = []
    for i, n in enumerate(names):
        d = g.read_config_file(voice_path(n, True))
        d.update({k: str(v) for k, v in ((overrides or {}).get(i) or {}).items()})
        out.append(g.config5_from_dict(d, rate, capi.PRECISION_F32))
    return out


def float_voices_plan(cfgs=None, rate=48000.0, rows=0, device=0, crate=250.0):
    return g.VoicesPlan(configs5f(rate) if cfgs is None else cfgs, crate, device, diagnostics=bool(rows), rows=rows, float_model5=True)


def single_float_plan(cfg, rows=0, device=0, crate=250.0):
    return g.Plan(cfg, crate, device, diagnostics=bool(rows), rows=rows, float_model5=True)


def create(cfgs, n=None, control_rate=250.0, entry="gvtm_plan_create_model5_float_voices", plan_out=True):
    """The entry for a design-only plan -> (status, handle, message); a plan that was made is destroyed again."""
    lib = g.load_library()
    h = ctypes.c_void_p()
    arr = (capi.Config5 * len(cfgs))(*cfgs) if cfgs else None
    rc = getattr(lib, entry)(arr, len(cfgs) if n is None else n, control_rate, capi.DEVICE_NONE, ctypes.byref(h) if plan_out else None)
    msg = lib.gvtm_last_error()
    if rc == 0:
        lib.gvtm_plan_destroy(h)
    return rc, h, msg


def singles_of(cfgs, params, ids, frames, rows=0):
    """Every utterance through a single-voice float plan of its voice: {b: (samples, count, maxabs)}."""
    out = {}
    for v, cfg in enumerate(cfgs):
        sel = np.nonzero(ids == v)[0]
        if sel.size == 0:
            continue
        audio, counts, maxabs = single_float_plan(cfg, rows).synthesize_host(params[sel], frames[sel])
        for j, b in enumerate(sel):
            out[int(b)] = (audio[j, : counts[j]].copy(), int(counts[j]), maxabs[j])
    return out


def assert_as_singles(audio, counts, maxabs, singles, ids, skip=()):
    """Bit identity of every utterance with its single-voice plan's: samples, count and maxabs (== abs(out).max())."""
    for b in range(len(ids)):
        if b in skip:
            continue
        ref, n, peak = singles[b]
        assert counts[b] == n, b
        assert within(audio[b, :n], ref, BIT_IDENTICAL), (b, int(ids[b]))
        assert maxabs[b] == peak == (np.abs(ref).max() if n else 0.0), b
