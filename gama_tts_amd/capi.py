"""ctypes binding of include/gama_vtm.h.  No computation happens here."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libgama_vtm.so"
N_PARAM = 16
DEVICE_NONE = -1
PRECISION_F64 = 0
PRECISION_MIXED = 1
PRECISION_F32 = 2  # everything in float, like the reference's TFloat = float models (model 1)
TUBE_10_6 = 0
TUBE_30_18 = 1
TABLE_FIR, TABLE_SRC_H, TABLE_SRC_DH, TABLE_WAVETABLE = 0, 1, 2, 3
_STATUS_UNSUPPORTED = 4


class GvtmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("gvtm status %d: %s" % (status, message))
        self.status = status


class Config(ctypes.Structure):
    _fields_ = [
        ("output_rate", ctypes.c_double),
        ("waveform", ctypes.c_int32),
        ("noise_modulation", ctypes.c_int32),
        ("glottal_pulse_tp", ctypes.c_double),
        ("glottal_pulse_tn_min", ctypes.c_double),
        ("glottal_pulse_tn_max", ctypes.c_double),
        ("breathiness", ctypes.c_double),
        ("vocal_tract_length_offset", ctypes.c_double),
        ("vocal_tract_length", ctypes.c_double),
        ("temperature", ctypes.c_double),
        ("loss_factor", ctypes.c_double),
        ("mouth_coefficient", ctypes.c_double),
        ("nose_coefficient", ctypes.c_double),
        ("throat_cutoff", ctypes.c_double),
        ("throat_volume", ctypes.c_double),
        ("mix_offset", ctypes.c_double),
        ("global_radius_coef", ctypes.c_double),
        ("global_nasal_radius_coef", ctypes.c_double),
        ("aperture_radius", ctypes.c_double),
        ("nasal_radius", ctypes.c_double * 5),
        ("radius_coef", ctypes.c_double * 8),
        ("section_delay", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("tube_layout", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
    ]


class Info(ctypes.Structure):
    _fields_ = [
        ("internal_sample_rate", ctypes.c_int32),
        ("control_steps", ctypes.c_uint32),
        ("output_rate", ctypes.c_double),
        ("control_rate", ctypes.c_double),
        ("fir_taps", ctypes.c_int32),
        ("time_register_increment", ctypes.c_uint32),
        ("phase_increment", ctypes.c_uint32),
        ("pad_size", ctypes.c_int32),
        ("upsampling", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("section_delay", ctypes.c_int32),
        ("model5", ctypes.c_int32),
        ("reserved_", ctypes.c_int32),
        ("internal_rate_hz", ctypes.c_double),
    ]


class Config5(ctypes.Structure):
    """gvtm5_config: VocalTractModel5's configuration keys (reference model 5)."""
    _fields_ = [
        ("output_rate", ctypes.c_double),
        ("waveform", ctypes.c_int32), ("noise_modulation", ctypes.c_int32), ("bypass", ctypes.c_int32),
        ("constant_radius_mouth_impedance", ctypes.c_int32),
        ("glottal_pulse_tp", ctypes.c_double), ("glottal_pulse_tn_min", ctypes.c_double),
        ("glottal_pulse_tn_max", ctypes.c_double), ("breathiness", ctypes.c_double),
        ("vocal_tract_length_offset", ctypes.c_double), ("vocal_tract_length", ctypes.c_double),
        ("temperature", ctypes.c_double), ("loss_factor", ctypes.c_double), ("mix_offset", ctypes.c_double),
        ("global_radius_coef", ctypes.c_double), ("global_nasal_radius_coef", ctypes.c_double),
        ("nasal_radius", ctypes.c_double * 6),
        ("radius_coef", ctypes.c_double * 8),
        ("glottal_noise_cutoff", ctypes.c_double), ("frication_noise_cutoff", ctypes.c_double),
        ("frication_factor", ctypes.c_double), ("min_glottal_loss", ctypes.c_double),
        ("max_glottal_loss", ctypes.c_double), ("glottal_lowpass_cutoff", ctypes.c_double),
        ("mouth_impedance_radius", ctypes.c_double),
        ("precision", ctypes.c_int32), ("reserved_", ctypes.c_int32),
    ]


class PackedStats(ctypes.Structure):
    """gvtm_packed_stats"""
    _fields_ = [("staging_bytes", ctypes.c_size_t), ("limit", ctypes.c_size_t), ("slices", ctypes.c_size_t),
                ("largest_slice", ctypes.c_size_t)]


class TrackConfig(ctypes.Structure):
    """gvtm_track_config"""
    _fields_ = [("control_period_ms", ctypes.c_int32), ("macro_intonation", ctypes.c_int32), ("micro_intonation", ctypes.c_int32),
                ("intonation_drift", ctypes.c_int32), ("smooth_intonation", ctypes.c_int32), ("reserved_", ctypes.c_int32),
                ("initial_pitch", ctypes.c_double), ("mean_pitch", ctypes.c_double), ("drift_deviation", ctypes.c_double),
                ("drift_sample_rate", ctypes.c_double), ("drift_lowpass_cutoff", ctypes.c_double)]


PACKED_ALIGN = 8  # GVTM_PACKED_ALIGN


def _prototypes():
    """The two prototype tables, name -> (restype, argtypes): every function include/gama_vtm.h declares, and every
    gvtm_debug_* hook csrc/vtm_capi_hooks.cpp defines.  A pointer to one of the structures above is typed; every other
    pointer is a c_void_p, which takes what _ptr() makes, a byref() and a ctypes array alike.  Written out, not derived:
    tests/test_capi_prototypes_cpu.py compares them with the C sources."""
    vp, sz, i, i64, dbl, text = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_char_p
    config, config5, info = ctypes.POINTER(Config), ctypes.POINTER(Config5), ctypes.POINTER(Info)
    tracks, stats = ctypes.POINTER(TrackConfig), ctypes.POINTER(PackedStats)
    product = {
        "gvtm_status_string": (text, [i]),
        "gvtm_last_error": (text, []),
        "gvtm_device_count": (i, []),
        "gvtm_plan_create": (i, [config, dbl, i, vp]),
        "gvtm_plan_create_model5": (i, [config5, dbl, i, vp]),
        "gvtm_plan_create_model5_float": (i, [config5, dbl, i, vp]),
        "gvtm_plan_destroy": (None, [vp]),
        "gvtm_plan_info": (i, [vp, info]),
        "gvtm_plan_table": (i, [vp, i, vp, sz]),
        "gvtm_output_count": (sz, [vp, sz]),
        "gvtm_output_capacity": (sz, [vp, sz]),
        "gvtm_synthesize_batch_device": (i, [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "gvtm_synthesize_batch_host": (i, [vp, vp, vp, sz, sz, vp, sz, vp, vp]),
        "gvtm_synthesize_batch_host_pcm16": (i, [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "gvtm_plan_create_voices": (i, [config, sz, dbl, i, vp]),
        "gvtm_plan_create_model5_voices": (i, [config5, sz, dbl, i, vp]),
        "gvtm_plan_create_model5_float_voices": (i, [config5, sz, dbl, i, vp]),
        "gvtm_plan_voice_count": (i, [vp]),
        "gvtm_plan_voice_info": (i, [vp, i, info]),
        "gvtm_voice_output_count": (sz, [vp, i, sz]),
        "gvtm_voices_output_capacity": (sz, [vp, sz]),
        "gvtm_synthesize_voices_device": (i, [vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "gvtm_synthesize_voices_host": (i, [vp, vp, vp, vp, sz, sz, vp, sz, vp, vp]),
        "gvtm_synthesize_voices_host_pcm16": (i, [vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "gvtm_packed_sample_offsets": (sz, [vp, vp, vp, sz, vp]),
        "gvtm_synthesize_packed_host": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp, vp]),
        "gvtm_synthesize_packed_host_pcm16": (i, [vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp]),
        "gvtm_plan_set_staging_limit": (i, [vp, sz]),
        "gvtm_plan_packed_stats": (i, [vp, stats]),
        "gvtm_plan_reserve": (i, [vp, sz]),
        "gvtm_host_alloc": (i, [sz, vp]),
        "gvtm_host_free": (None, [vp]),
        "gvtm_stream_create": (i, [vp, sz, vp]),
        "gvtm_stream_create_voices": (i, [vp, vp, sz, vp]),
        "gvtm_stream_destroy": (None, [vp]),
        "gvtm_stream_reset": (i, [vp]),
        "gvtm_stream_reset_voices": (i, [vp, vp]),
        "gvtm_stream_capacity": (sz, [vp, sz]),
        "gvtm_stream_push": (i, [vp, vp, vp, sz, vp, sz, vp]),
        "gvtm_stream_finish": (i, [vp, vp, sz, vp, vp]),
        "gvtm_normalize_batch_device": (i, [vp, vp, sz, sz, vp, vp, vp, vp, vp, vp]),
        "gvtm_plan_set_timing": (i, [vp, i]),
        "gvtm_plan_take_kernel_ms": (dbl, [vp, vp]),
        "gvtm_tracks_frame_count": (sz, [tracks, vp, sz]),
        "gvtm_generate_tracks_device": (i, [i, tracks, vp, vp, sz, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_events_device": (i, [vp, tracks, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]),
        "gvtm_plan_set_voice_tracks": (i, [vp, tracks, sz]),
        "gvtm_generate_tracks_voices_device": (i, [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_events_voices_device": (i, [vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]),
        "gvtm_tracks_chunks_frame_count": (sz, [tracks, vp, vp, sz]),
        "gvtm_generate_tracks_chunks_device": (i, [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_events_chunks_device": (i, [vp, vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]),
        "gvtm_intonation_apply_host": (i64, [tracks, vp, sz, vp, sz, vp, sz, vp]),
        "gvtm_apply_intonation_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp]),
        "gvtm_synthesize_intonation_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, sz, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp]),
        "gvtm_modification_filter_length": (i64, [vp, i]),
        "gvtm_modification_apply_host": (i, [vp, i, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "gvtm_apply_modifications_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_modified_device": (i, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]),
        "gvtm_targets_filter_length": (i64, [vp, i]),
        "gvtm_targets_output_count": (sz, [vp, sz]),
        "gvtm_targets_output_capacity": (sz, [vp, sz]),
        "gvtm_targets_apply_host": (i, [vp, i, vp, vp, vp, i64, vp, vp]),
        "gvtm_targets_apply_host_from": (i, [vp, i, vp, vp, vp, i64, i64, vp, vp, vp]),
        "gvtm_synthesize_targets_device": (i, [vp, vp, sz, vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_targets_model5_device": (i, [vp, vp, sz, vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp]),
        "gvtm_targets_voice_output_count": (sz, [vp, i, sz]),
        "gvtm_targets_voices_output_capacity": (sz, [vp, sz]),
        "gvtm_synthesize_targets_voices_device": (i, [vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_targets_model5_voices_device": (i, [vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp]),
        "gvtm_stream_push_targets": (i, [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "gvtm_stream_push_targets_model5": (i, [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "gvtm_stream_push_targets_voices": (i, [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "gvtm_stream_push_targets_model5_voices": (i, [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp]),
        "gvtm_stream_targets_capacity": (sz, [vp, sz]),
        "gvtm_stream_targets_points": (i, [vp, vp]),
        "gvtm_stream_push_events": (i, [vp, vp, vp, vp, vp, sz, vp, vp]),
        "gvtm_stream_get_drift": (i, [vp, vp]),
        "gvtm_stream_set_drift": (i, [vp, vp]),
        "gvtm_events_packed_layout": (sz, [vp, vp, vp, vp, vp, sz, vp, vp]),
        "gvtm_synthesize_events_packed_host": (i, [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp]),
        "gvtm_synthesize_events_packed_host_pcm16": (i, [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp]),
        "gvtm_generate_tracks_host": (i, [i, tracks, vp, vp, sz, sz, vp, vp, vp]),
        "gvtm_analysis_create": (i, [i, vp, vp]),
        "gvtm_analysis_destroy": (None, [vp]),
        "gvtm_analysis_bin_count": (sz, [vp]),
        "gvtm_analysis_window": (i, [vp, vp, sz]),
        "gvtm_analysis_buffer_count": (sz, [i64, i64, sz]),
        "gvtm_analysis_reserve": (i, [vp, sz]),
        "gvtm_analysis_apply_host": (i, [vp, vp, sz, sz, sz, vp, vp, vp]),
        "gvtm_analyze_spectrum_device": (i, [vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp]),
        "gvtm_listen_buffer_count": (sz, [i64, i64, vp]),
        "gvtm_stream_listen": (i, [vp, vp, sz, i]),
        "gvtm_stream_unlisten": (i, [vp]),
        "gvtm_stream_listen_state": (i, [vp, vp, vp]),
        "gvtm_stream_take_spectra": (i, [vp, vp, vp, vp]),
        "gvtm_stream_peek_spectra_device": (i, [vp, vp, vp, vp]),
        "gvtm_rules_create": (i, [i, vp, vp]),
        "gvtm_rules_destroy": (None, [vp]),
        "gvtm_rules_apply_host": (i, [vp, i, vp, sz, vp, sz, vp, vp, sz, vp, vp, vp]),
        "gvtm_rules_event_count": (i64, [vp, i, vp, sz, vp]),
        "gvtm_generate_events_device": (i, [vp, i, vp, vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "gvtm_synthesize_postures_device": (i, [vp, vp, tracks, vp, vp, sz, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp]),
        "gvtm_prosody_create": (i, [i, vp, vp, sz, vp]),
        "gvtm_prosody_destroy": (None, [vp]),
        "gvtm_prosody_rhythm_host": (i, [vp, vp, sz, vp, sz, vp, vp]),
        "gvtm_prosody_point_count": (i64, [sz, vp, sz, vp, sz]),
        "gvtm_prosody_points_host": (i, [vp, i, vp, sz, vp, sz, vp, sz, vp, vp, sz, vp, i, vp, sz, vp, vp]),
        "gvtm_apply_rhythm_device": (i, [vp, vp, vp, sz, vp, vp, sz, sz, vp, vp, vp]),
        "gvtm_place_intonation_device": (i, [vp, i, vp, vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp]),
        "gvtm_synthesize_prosody_device": (i, [vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, sz, sz, sz, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
    }
    hooks = {
        "gvtm_debug_set_rows": (i, [vp, i]),
        "gvtm_debug_lds_bytes": (sz, [vp, i]),
        "gvtm_debug_launch_shape": (i, [vp, sz, i, vp]),
        "gvtm_debug_stream_launch_shape": (i, [vp, sz, vp]),
        "gvtm_debug_chunk_length": (i, [vp, sz]),
        "gvtm_debug_plan_filter_split": (i, [vp, i]),
        "gvtm_debug_fir_literals": (i, [vp]),
        "gvtm_debug_plan_fir_literals": (i, [vp]),
        "gvtm_debug_force_generic_fir": (i, [vp]),
        "gvtm_debug_plan_src_phases": (i, [vp]),
        "gvtm_debug_plan_src_phase_table": (i, [vp, vp, sz]),
        "gvtm_debug_force_generic_src": (i, [vp]),
        "gvtm_debug_plan_static_wavetable": (i, [vp]),
        "gvtm_debug_force_dynamic_wavetable": (i, [vp]),
        "gvtm_debug_noise_table": (i, [sz, i, vp]),
        "gvtm_debug_set_taps": (i, [vp, vp]),
        "gvtm_debug_set_phase_cycles": (i, [vp, vp]),
        "gvtm_debug_dpp_selftest": (i, [vp, vp]),
        "gvtm_debug_short_math": (i, [i, vp, sz, vp]),
        "gvtm_debug_device_float_math": (i, [vp, i, vp, sz, vp]),
        "gvtm_debug_group_voices": (i, [vp, vp, sz, i, vp, vp, vp, vp]),
        "gvtm_debug_tracks_append": (i, [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, vp]),
        "gvtm_debug_tracks_slice": (i, [vp, vp, i64, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp]),
        "gvtm_debug_carry_rows": (i, [vp, vp, vp, vp, sz, sz]),
        "gvtm_debug_listen_copy": (i, [i, vp, sz, vp, sz, vp, vp, vp, sz, i64]),
        "gvtm_debug_listen_move": (i, [i64, i64, vp]),
        "gvtm_debug_stream_targets_sums": (i, [vp, vp]),
        "gvtm_debug_analyze_slots": (i, [vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
        "gvtm_debug_analysis_float_host": (i, [vp, vp, vp]),
    }
    return product, hooks


PROTOTYPES, HOOK_PROTOTYPES = _prototypes()
# what every build of the library has had; the rest came later, and a variant built from an older commit (GVTM_LIBRARY,
# tools/ab.py) that lacks some of it still loads: such an entry fails when it is called
_REQUIRED = (
    "gvtm_status_string", "gvtm_last_error", "gvtm_device_count", "gvtm_plan_create", "gvtm_plan_create_model5", "gvtm_plan_destroy",
    "gvtm_plan_info", "gvtm_plan_table", "gvtm_output_count", "gvtm_output_capacity", "gvtm_synthesize_batch_device",
    "gvtm_synthesize_batch_host", "gvtm_synthesize_batch_host_pcm16", "gvtm_host_alloc", "gvtm_host_free", "gvtm_normalize_batch_device",
    "gvtm_tracks_frame_count", "gvtm_generate_tracks_device", "gvtm_synthesize_events_device", "gvtm_generate_tracks_host",
    "gvtm_stream_create", "gvtm_stream_destroy", "gvtm_stream_reset", "gvtm_stream_capacity", "gvtm_stream_push", "gvtm_stream_finish",
    "gvtm_plan_set_timing", "gvtm_plan_take_kernel_ms")


def library_path(diagnostics=False):
    return os.path.join(_HERE, "lib", "libgama_vtm_diag.so" if diagnostics else _LIB_NAME)


_libs = {}


def load_library(diagnostics=False):
    """Loads libgama_vtm.so from the in-tree build; raises if it has not been built.

    diagnostics=True loads libgama_vtm_diag.so instead: the same kernels behind a C ABI built with -DGVTM_DIAGNOSTICS,
    which adds the gvtm_debug_* hooks (tests and tools only; the product library exports none of them)."""
    if diagnostics in _libs:
        return _libs[diagnostics]
    # GVTM_LIBRARY / GVTM_DIAG_LIBRARY: A/B runs of library variants (tools/ab.py; tools/build_variant.sh builds one with
    # csrc/Makefile's recipe: the diagnostics library under extra flags, in gama_tts_amd/lib_variants/)
    path = (os.environ.get("GVTM_DIAG_LIBRARY") or library_path(True)) if diagnostics else (os.environ.get("GVTM_LIBRARY") or library_path())
    # libgama_vtm.so and PyTorch-ROCm both need libamdhip64.so.7 and a process can hold only one
    # copy: whichever loads first serves both.  PyTorch only works with the copy bundled in its
    # wheel, so when torch is installed let it load first (bench.py/tests share device pointers
    # and streams with torch).  C/C++ hosts are unaffected: they use the system ROCm runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C gama_tts_amd/csrc). There is no fallback path." % path)
    lib = ctypes.CDLL(path)
    table = {**PROTOTYPES, **HOOK_PROTOTYPES} if diagnostics else PROTOTYPES
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name, None)  # None: a variant from before the entry existed
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
        elif name in _REQUIRED:
            raise ImportError("%s does not export %s: it is no build of include/gama_vtm.h. There is no fallback path." % (path, name))
    _libs[diagnostics] = lib
    return lib


def _check(lib, rc):
    """Raises GvtmError for a status other than 0, with the failing call's message or else the status's name."""
    if rc != 0:
        raise GvtmError(rc, lib.gvtm_last_error().decode() or lib.gvtm_status_string(rc).decode())


def _count(lib, n):
    """The result of an entry that returns a size_t, (size_t)-1 for a refused call."""
    if n == ctypes.c_size_t(-1).value:
        raise GvtmError(1, lib.gvtm_last_error().decode())
    return n


def fir_literal_table():
    """The 47 float coefficients the float kernels hold as literals (diagnostics library)."""
    out = np.empty(47, dtype=np.float32)
    n = load_library(True).gvtm_debug_fir_literals(out.ctypes.data)
    assert n == out.size, n
    return out


def device_count():
    return int(load_library().gvtm_device_count())


class PinnedArray:
    """A numpy array over page-locked host memory from gvtm_host_alloc (the buffers of the host entries: with them the
    H2D / kernel / D2H pipeline really overlaps).  Keep the object alive as long as `.array` is in use."""

    def __init__(self, shape, dtype):
        self._lib = load_library()
        self.array = None
        self._ptr = ctypes.c_void_p()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _check(self._lib, self._lib.gvtm_host_alloc(max(nbytes, 1), ctypes.byref(self._ptr)))
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(self._ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self._ptr:
            self.array = None
            self._lib.gvtm_host_free(self._ptr)
            self._ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_config_file(path):
    """`key = value` lines, `#` comments — the reference's ConfigurationData file format
    (gama_tts/src/ConfigurationData.cpp:67-118)."""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if not line or line.startswith("#"):
                continue
            key, value = line.split("=", 1)
            out[key.strip()] = value.strip()
    return out


def config_from_dict(d, output_rate=None, section_delay=1, precision=PRECISION_F64, tube_layout=TUBE_10_6):
    """Builds a gvtm_config from the merged vtm.txt + variant keys (VocalTractModel0.h:266-305)."""
    c = Config()
    c.output_rate = float(d["output_rate"]) if output_rate is None else float(output_rate)
    c.waveform = int(float(d["waveform"]))
    c.noise_modulation = int(float(d["noise_modulation"]))
    for key in ("glottal_pulse_tp", "glottal_pulse_tn_min", "glottal_pulse_tn_max", "breathiness",
                "vocal_tract_length_offset", "vocal_tract_length", "temperature", "loss_factor",
                "mouth_coefficient", "nose_coefficient", "throat_cutoff", "throat_volume", "mix_offset",
                "global_radius_coef", "global_nasal_radius_coef", "aperture_radius"):
        setattr(c, key, float(d[key]))
    for i in range(5):
        c.nasal_radius[i] = float(d["nasal_radius_%d" % (i + 1)])
    for i in range(8):
        c.radius_coef[i] = float(d["radius_%d_coef" % (i + 1)])
    c.section_delay = int(section_delay)
    c.precision = int(precision)
    c.tube_layout = int(tube_layout)
    return c


def config5_from_dict(d, output_rate=None, precision=PRECISION_F64):
    """Builds a gvtm5_config from the merged vtm.txt + variant keys of a model-5 voice (VocalTractModel5.h:375-421)."""
    c = Config5()
    c.output_rate = float(d["output_rate"]) if output_rate is None else float(output_rate)
    for key in ("waveform", "noise_modulation", "bypass"):
        setattr(c, key, int(float(d[key])))
    c.constant_radius_mouth_impedance = 1 if str(d["constant_radius_mouth_impedance"]).strip().lower() in ("1", "true") else 0
    for key in ("glottal_pulse_tp", "glottal_pulse_tn_min", "glottal_pulse_tn_max", "breathiness",
                "vocal_tract_length_offset", "vocal_tract_length", "temperature", "loss_factor", "mix_offset",
                "global_radius_coef", "global_nasal_radius_coef", "glottal_noise_cutoff", "frication_noise_cutoff",
                "frication_factor", "min_glottal_loss", "max_glottal_loss", "glottal_lowpass_cutoff"):
        setattr(c, key, float(d[key]))
    c.mouth_impedance_radius = float(d.get("mouth_impedance_radius", 0.0))
    for i in range(6):
        c.nasal_radius[i] = float(d["nasal_radius_%d" % (i + 2)])
    for i in range(8):
        c.radius_coef[i] = float(d["radius_%d_coef" % (i + 1)])
    c.precision = int(precision)
    return c


# gvtm_event / gvtm_drift_state as numpy record layouts
EVENT_DTYPE = np.dtype([("time_ms", "<i4"), ("has_interp", "<i4"), ("interp", "<f8", 4), ("param", "<f8", 16),
                        ("special", "<f8", 16)])
DRIFT_DTYPE = np.dtype([("seed", "<f8"), ("x1", "<f8"), ("x2", "<f8"), ("y1", "<f8"), ("y2", "<f8")])
FRESH_DRIFT = (0.7892347, 0.0, 0.0, 0.0, 0.0)


def events_from_table(table):
    """float64 [E][38] rows (time, has_interp, a, b, c, d, parameters[16], specialParameters[16]) -> gvtm_event records."""
    table = np.asarray(table, dtype=np.float64)
    ev = np.zeros(table.shape[0], dtype=EVENT_DTYPE)
    ev["time_ms"] = table[:, 0].astype(np.int32)
    ev["has_interp"] = (table[:, 1] != 0).astype(np.int32)
    ev["interp"] = table[:, 2:6]
    ev["param"] = table[:, 6:22]
    ev["special"] = table[:, 22:38]
    return ev


def tracks_frame_count(config, events):
    lib = load_library()
    events = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    return _count(lib, lib.gvtm_tracks_frame_count(ctypes.byref(config), _ptr(events), events.shape[0]))


def tracks_chunks_frame_count(config, events, chunk_offsets):
    """gvtm_tracks_chunks_frame_count: the frames of one utterance whose chunk c owns events[chunk_offsets[c]:chunk_offsets[c + 1]]."""
    lib = load_library()
    events = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    chunk_offsets = np.ascontiguousarray(chunk_offsets, dtype=np.int64)
    return _count(lib, lib.gvtm_tracks_chunks_frame_count(ctypes.byref(config), _ptr(events), _ptr(chunk_offsets),
                                                          max(chunk_offsets.shape[0] - 1, 0)))


# gvtm_intonation_point as a numpy record layout (24 bytes)
POINT_DTYPE = np.dtype([("time_ms", "<f8"), ("semitone", "<f8"), ("slope", "<f8")])
MAX_INTONATION_POINTS = 64  # GVTM_MAX_INTONATION_POINTS


def points_from_table(table):
    """float64 [P][3] rows (time_ms, semitone, slope) -> gvtm_intonation_point records."""
    return np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1, 3)).view(POINT_DTYPE).reshape(-1)


def intonation_apply_host(config, events, points, count_only=False, capacity=None):
    """gvtm_intonation_apply_host: gvtm_event records and gvtm_intonation_point records -> (merged gvtm_event records, or
    with count_only their number; status).  A refused utterance has no merged events and a status other than 0.
    capacity: events the output is sized for (default: len(events) + len(points), which always holds them)."""
    lib = load_library()
    events = np.ascontiguousarray(events, dtype=EVENT_DTYPE)
    points = np.ascontiguousarray(points, dtype=POINT_DTYPE)
    status = ctypes.c_int32(-1)
    capacity = events.shape[0] + points.shape[0] if capacity is None else int(capacity)
    out = None if count_only else np.zeros(max(capacity, 1), dtype=EVENT_DTYPE)
    n = lib.gvtm_intonation_apply_host(ctypes.byref(config), _ptr(events), events.shape[0], _ptr(points), points.shape[0], _ptr(out),
                                       capacity, ctypes.byref(status))
    if n < 0:
        raise GvtmError(1, lib.gvtm_last_error().decode())
    return (int(n) if count_only else out[:n].copy()), int(status.value)


# gvtm_posture and gvtm_rule_data as numpy record layouts (24 and 48 bytes)
POSTURE_DTYPE = np.dtype([("posture", "<i4"), ("marked", "<i4"), ("tempo", "<f8"), ("rule_tempo", "<f8")])
RULE_DATA_DTYPE = np.dtype([("number", "<i4"), ("first_posture", "<i4"), ("last_posture", "<i4"), ("start", "<i4"), ("mark1", "<f8"),
                            ("mark2", "<f8"), ("duration", "<f8"), ("beat", "<f8")])
RULES_OK, RULES_NO_RULE, RULES_TOO_SMALL, RULES_BAD_VALUE, RULES_BAD_POSTURE, RULES_NO_ROOM = range(6)  # the statuses of the rule


class RulesModel(ctypes.Structure):
    """gvtm_rules_model: eight counts, then the arrays (control_model.ARRAYS names them as the header does)."""
    _COUNTS = ("n_postures", "n_rules", "n_equations", "n_program_ops", "n_transitions", "n_items", "n_points", "n_slopes")
    _ARRAYS = (("param_target", np.float32), ("symbol_target", np.float32), ("param_min", np.float32), ("param_max", np.float32),
               ("rule_n_expr", np.int32), ("rule_equations", np.int32), ("rule_param_transition", np.int32),
               ("rule_special_transition", np.int32), ("match", np.uint8), ("equation_offsets", np.int32), ("program_op", np.int32),
               ("program_const", np.float32), ("transition_offsets", np.int32), ("items", np.int32), ("point_type", np.int32),
               ("point_value", np.float32), ("point_free_time", np.float32), ("point_time_eq", np.int32), ("slopes", np.float32))
    _fields_ = [(n, ctypes.c_int32) for n in _COUNTS] + [(n, ctypes.c_void_p) for n, _ in _ARRAYS]


def postures_from_table(table):
    """rows (posture id, marked, tempo, rule_tempo) -> gvtm_posture records."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(table.shape[0], dtype=POSTURE_DTYPE)
    out["posture"], out["marked"], out["tempo"], out["rule_tempo"] = table[:, 0].astype(np.int32), table[:, 1].astype(np.int32), table[:, 2], table[:, 3]
    return out


class Rules:
    """Owns a gvtm_rules: a compiled articulatory model (the arrays of control_model.compile_model, or of an .npz written from
    them), checked and, unless device is DEVICE_NONE, uploaded."""

    def __init__(self, model, device=DEVICE_NONE):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        arrays = {name: np.ascontiguousarray(model[name], dtype=dtype) for name, dtype in RulesModel._ARRAYS}
        m = RulesModel()
        m.n_postures, m.n_rules = arrays["param_target"].shape[0], arrays["rule_n_expr"].shape[0]
        m.n_equations, m.n_program_ops = arrays["equation_offsets"].shape[0] - 1, arrays["program_op"].shape[0]
        m.n_transitions, m.n_items = arrays["transition_offsets"].shape[0] - 1, arrays["items"].size // 5
        m.n_points, m.n_slopes = arrays["point_type"].shape[0], arrays["slopes"].shape[0]
        for name, _ in RulesModel._ARRAYS:
            setattr(m, name, arrays[name].ctypes.data)
        self.n_postures, self.device = int(m.n_postures), int(device)
        _check(self._lib, self._lib.gvtm_rules_create(int(device), ctypes.byref(m), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gvtm_rules_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def event_count(self, control_period, postures):
        """gvtm_rules_event_count -> (events, status)."""
        postures = np.ascontiguousarray(postures, dtype=POSTURE_DTYPE)
        status = ctypes.c_int32(-1)
        n = self._lib.gvtm_rules_event_count(self._h, int(control_period), _ptr(postures), postures.shape[0], ctypes.byref(status))
        if n < 0:
            raise GvtmError(1, self._lib.gvtm_last_error().decode())
        return int(n), int(status.value)

    def apply_host(self, control_period, postures, capacity=None, rule_capacity=None):
        """gvtm_rules_apply_host: gvtm_posture records -> (gvtm_event records, gvtm_rule_data records, onsets float64 [n],
        status).  A refused utterance has no events and no rule data.  capacity: events the output is sized for (default:
        what gvtm_rules_event_count says); rule_capacity: rows of rule data (default: one per posture)."""
        postures = np.ascontiguousarray(postures, dtype=POSTURE_DTYPE)
        n = postures.shape[0]
        capacity = self.event_count(control_period, postures)[0] if capacity is None else int(capacity)
        rule_capacity = n if rule_capacity is None else int(rule_capacity)
        events = np.zeros(max(capacity, 1), dtype=EVENT_DTYPE)
        rule_data = np.zeros(max(rule_capacity, 1), dtype=RULE_DATA_DTYPE)
        onsets = np.zeros(max(n, 1), dtype=np.float64)
        n_events, n_rules, status = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int32(-1)
        _check(self._lib, self._lib.gvtm_rules_apply_host(self._h, int(control_period), _ptr(postures), n, _ptr(events), capacity, ctypes.byref(n_events),
                                                         _ptr(rule_data), rule_capacity, ctypes.byref(n_rules), _ptr(onsets), ctypes.byref(status)))
        return events[: n_events.value].copy(), rule_data[: min(n_rules.value, rule_capacity)].copy(), onsets[:n], int(status.value)

    def generate_events_device(self, control_period, d_postures, d_posture_offsets, batch, d_events_out, out_capacity, d_event_offsets_out,
                               d_rule_data=None, max_rules=0, d_rule_counts=None, d_onsets=None, d_status=None, stream=None):
        """gvtm_generate_events_device: posture sequences -> event lists, their offsets, rule data, onsets and statuses; all
        pointers are device memory."""
        _check(self._lib, self._lib.gvtm_generate_events_device(
            self._h, int(control_period), _ptr(d_postures), _ptr(d_posture_offsets), int(batch), _ptr(d_events_out), int(out_capacity),
            _ptr(d_event_offsets_out), _ptr(d_rule_data), int(max_rules), _ptr(d_rule_counts), _ptr(d_onsets), _ptr(d_status), _ptr(stream)))


# gvtm_foot, gvtm_tone_group and gvtm_prosody_config as numpy record layouts (24, 32 and 112 bytes)
FOOT_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("marked", "<i4"), ("reserved_", "<i4"), ("tempo", "<f8")])
TONE_GROUP_DTYPE = np.dtype([("start_foot", "<i4"), ("end_foot", "<i4"), ("type", "<i4"), ("param", "<f4", 5)])
PROSODY_INTONATION_KEYS = ("time_offset", "pretonic_base_slope", "pretonic_base_slope_random", "pretonic_slope_random_factor", "tonic_base_slope",
                           "tonic_continuation_base_slope", "tonic_slope_random_factor", "tonic_slope_offset")  # intonation.txt
PROSODY_RHYTHM_KEYS = ("marked_a", "marked_b", "marked_div", "unmarked_a", "unmarked_b", "unmarked_div", "min_tempo", "max_tempo")  # rhythm.txt
PROSODY_CONFIG_DTYPE = np.dtype([(k, "<f4") for k in PROSODY_INTONATION_KEYS] + [("intonation_factor", "<f4"), ("reserved_", "<f4")] +
                                [(k, "<f8") for k in PROSODY_RHYTHM_KEYS] + [("global_tempo", "<f8")])
PROSODY_OK, PROSODY_BAD_STRUCTURE, PROSODY_NO_RULES, PROSODY_TOO_MANY, PROSODY_BAD_VALUE, PROSODY_NO_ROOM = range(6)  # the statuses of the two rules
TONE_GROUP_CONTINUATION, TONE_GROUP_NONE = 3, 5


def feet_from_table(table):
    """rows (start, end, marked, tempo) -> gvtm_foot records."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(table.shape[0], dtype=FOOT_DTYPE)
    out["start"], out["end"], out["marked"], out["tempo"] = table[:, 0].astype(np.int32), table[:, 1].astype(np.int32), table[:, 2].astype(np.int32), table[:, 3]
    return out


def tone_groups_from_table(table):
    """rows (start_foot, end_foot, type, param[5]) -> gvtm_tone_group records (the parameters rounded to float once)."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 8)
    out = np.zeros(table.shape[0], dtype=TONE_GROUP_DTYPE)
    out["start_foot"], out["end_foot"], out["type"] = table[:, 0].astype(np.int32), table[:, 1].astype(np.int32), table[:, 2].astype(np.int32)
    out["param"] = table[:, 3:8].astype(np.float32)
    return out


def prosody_config(intonation, rhythm, intonation_factor=1.0, global_tempo=1.0):
    """The eight floats of intonation.txt and the eight doubles of rhythm.txt (dicts by the files' keys, or sequences in
    PROSODY_INTONATION_KEYS / PROSODY_RHYTHM_KEYS order) with the two factors -> one gvtm_prosody_config record."""
    out = np.zeros((), dtype=PROSODY_CONFIG_DTYPE)
    for keys, values in ((PROSODY_INTONATION_KEYS, intonation), (PROSODY_RHYTHM_KEYS, rhythm)):
        for k, key in enumerate(keys):
            out[key] = values[key] if isinstance(values, dict) else values[k]
    out["intonation_factor"], out["global_tempo"] = intonation_factor, global_tempo
    return out


def prosody_point_count(n_postures, feet, groups):
    """gvtm_prosody_point_count: the points the tables alone promise, or -1 for a structure the rule refuses."""
    lib = load_library()
    feet, groups = np.ascontiguousarray(feet, dtype=FOOT_DTYPE), np.ascontiguousarray(groups, dtype=TONE_GROUP_DTYPE)
    return int(lib.gvtm_prosody_point_count(int(n_postures), _ptr(feet), feet.shape[0], _ptr(groups), groups.shape[0]))


class Prosody:
    """Owns a gvtm_prosody: a gvtm_prosody_config record (prosody_config) and the model's vocoid table
    (control_model.compile_model(...)["vocoid"]; None, a model without the category, is refused), checked and, unless device
    is DEVICE_NONE, uploaded."""

    def __init__(self, config, vocoid, device=DEVICE_NONE):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        config = np.ascontiguousarray(config, dtype=PROSODY_CONFIG_DTYPE).reshape(1)
        table = None if vocoid is None else np.ascontiguousarray(vocoid, dtype=np.uint8)
        self.device = int(device)
        _check(self._lib, self._lib.gvtm_prosody_create(int(device), _ptr(config), _ptr(table), 0 if table is None else table.shape[0], ctypes.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gvtm_prosody_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rhythm_host(self, postures, feet, in_place=False):
        """gvtm_prosody_rhythm_host: gvtm_posture and gvtm_foot records -> (the postures after rhythm, status)."""
        postures, feet = np.array(postures, dtype=POSTURE_DTYPE), np.ascontiguousarray(feet, dtype=FOOT_DTYPE)
        out = postures if in_place else np.zeros(max(postures.shape[0], 1), dtype=POSTURE_DTYPE)
        status = ctypes.c_int32(-1)
        _check(self._lib, self._lib.gvtm_prosody_rhythm_host(self._h, _ptr(postures), postures.shape[0], _ptr(feet), feet.shape[0], _ptr(out), ctypes.byref(status)))
        return out[: postures.shape[0]], int(status.value)

    def points_host(self, control_period, postures, feet, groups, draws, rule_data, onsets, rule_status=0, capacity=MAX_INTONATION_POINTS):
        """gvtm_prosody_points_host: the postures after rhythm, the tables, the draws (float64 [feet][2] or None) and what
        the rules entry left -> (gvtm_intonation_point records, status)."""
        postures, feet = np.ascontiguousarray(postures, dtype=POSTURE_DTYPE), np.ascontiguousarray(feet, dtype=FOOT_DTYPE)
        groups, rule_data = np.ascontiguousarray(groups, dtype=TONE_GROUP_DTYPE), np.ascontiguousarray(rule_data, dtype=RULE_DATA_DTYPE)
        onsets = np.ascontiguousarray(onsets, dtype=np.float64)
        draws = None if draws is None else np.ascontiguousarray(draws, dtype=np.float64).reshape(feet.shape[0], 2)
        points = np.zeros(max(int(capacity), 1), dtype=POINT_DTYPE)
        n_points, status = ctypes.c_size_t(0), ctypes.c_int32(-1)
        _check(self._lib, self._lib.gvtm_prosody_points_host(
            self._h, int(control_period), _ptr(postures), postures.shape[0], _ptr(feet), feet.shape[0], _ptr(groups), groups.shape[0], _ptr(draws),
            _ptr(rule_data), rule_data.shape[0], _ptr(onsets), int(rule_status), _ptr(points), int(capacity), ctypes.byref(n_points), ctypes.byref(status)))
        return points[: n_points.value].copy(), int(status.value)

    def apply_rhythm_device(self, d_postures, d_posture_offsets, n_postures, d_feet, d_foot_offsets, n_feet, batch, d_postures_out, d_status=None, stream=None):
        """gvtm_apply_rhythm_device; all pointers are device memory (d_postures_out may be d_postures)."""
        _check(self._lib, self._lib.gvtm_apply_rhythm_device(self._h, _ptr(d_postures), _ptr(d_posture_offsets), int(n_postures), _ptr(d_feet), _ptr(d_foot_offsets),
                                                             int(n_feet), int(batch), _ptr(d_postures_out), _ptr(d_status), _ptr(stream)))

    def place_intonation_device(self, control_period, d_postures, d_posture_offsets, d_feet, d_foot_offsets, d_groups, d_group_offsets, d_draws, batch,
                                d_rule_data, max_rules, d_rule_counts, d_onsets, d_points_out, points_capacity, d_point_offsets_out, d_status=None, stream=None):
        """gvtm_place_intonation_device: what gvtm_generate_events_device left -> points, their offsets and statuses."""
        _check(self._lib, self._lib.gvtm_place_intonation_device(
            self._h, int(control_period), _ptr(d_postures), _ptr(d_posture_offsets), _ptr(d_feet), _ptr(d_foot_offsets), _ptr(d_groups), _ptr(d_group_offsets),
            _ptr(d_draws), int(batch), _ptr(d_rule_data), int(max_rules), _ptr(d_rule_counts), _ptr(d_onsets), _ptr(d_points_out), int(points_capacity),
            _ptr(d_point_offsets_out), _ptr(d_status), _ptr(stream)))


MODIFICATION_ADD, MODIFICATION_MULTIPLY = 0, 1  # GVTM_MODIFICATION_*
MAX_GESTURES = 64  # GVTM_MAX_GESTURES


def pack_gestures(utterances):
    """utterances[b]: the gestures of utterance b, each (parameter, operation, steps, values) -> (gestures int32 [G][2],
    gesture_offsets int64 [G + 1], utt_gestures int64 [B + 1], point_steps int32, point_values float32): the tables of the
    modification entries, the points of all gestures back to back."""
    flat = [g for u in utterances for g in u]
    gestures = np.array([[int(g[0]), int(g[1])] for g in flat], dtype=np.int32).reshape(-1, 2)
    steps = [np.asarray(g[2], dtype=np.int32).reshape(-1) for g in flat]
    values = [np.asarray(g[3], dtype=np.float32).reshape(-1) for g in flat]
    assert all(s.shape == v.shape for s, v in zip(steps, values))
    gesture_offsets = np.zeros(len(flat) + 1, dtype=np.int64)
    gesture_offsets[1:] = np.cumsum([len(s) for s in steps])
    utt_gestures = np.zeros(len(utterances) + 1, dtype=np.int64)
    utt_gestures[1:] = np.cumsum([len(u) for u in utterances])
    point_steps = np.concatenate(steps) if steps else np.zeros(0, np.int32)
    point_values = np.concatenate(values) if values else np.zeros(0, np.float32)
    return gestures, gesture_offsets, utt_gestures, np.ascontiguousarray(point_steps), np.ascontiguousarray(point_values)


def modification_apply_host(plan, frames, gestures, voice=0, frames_out=None):
    """gvtm_modification_apply_host: base frames float32 [F][16] under `gestures` (a list of (parameter, operation, steps,
    values)) with the control steps and filter length of voice `voice` of `plan` -> (modified frames float32 [F][16],
    status).  A refused utterance leaves frames_out (by default zeros) as it was."""
    frames = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, N_PARAM)
    table, offsets, _, steps, values = pack_gestures([gestures])
    out = np.zeros_like(frames) if frames_out is None else frames_out
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= frames.size
    status = ctypes.c_int32(-1)
    _check(plan._lib, plan._lib.gvtm_modification_apply_host(plan._h, int(voice), _ptr(frames), frames.shape[0], _ptr(table), _ptr(offsets),
                                                             len(gestures), _ptr(steps), _ptr(values), _ptr(out), ctypes.byref(status)))
    return out, int(status.value)


def pack_targets(lists):
    """lists[l]: one list of points, (steps, values) -> (list_offsets int64 [L + 1], point_steps int32, point_values
    float32): the tables of the targets entries, the points of all lists back to back.  (An utterance's 16 lists, or a batch's
    lists with the ids that name them.)"""
    steps = [np.asarray(l[0], dtype=np.int32).reshape(-1) for l in lists]
    values = [np.asarray(l[1], dtype=np.float32).reshape(-1) for l in lists]
    assert all(s.shape == v.shape for s, v in zip(steps, values))
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in steps])
    point_steps = np.concatenate(steps) if steps else np.zeros(0, np.int32)
    point_values = np.concatenate(values) if values else np.zeros(0, np.float32)
    return offsets, np.ascontiguousarray(point_steps), np.ascontiguousarray(point_values)


def targets_apply_host(plan, lists, n_steps, voice=0, frames_out=None):
    """gvtm_targets_apply_host: the 16 lists of one utterance, each (steps, values), through the 50 ms filter of voice `voice`
    of `plan` -> (the parameters by step float32 [n_steps][16], status).  A refused utterance leaves frames_out (by default
    zeros) as it was."""
    assert len(lists) == N_PARAM
    offsets, steps, values = pack_targets(lists)
    out = np.zeros((max(int(n_steps), 0), N_PARAM), dtype=np.float32) if frames_out is None else frames_out
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= max(int(n_steps), 0) * N_PARAM
    status = ctypes.c_int32(-1)
    _check(plan._lib, plan._lib.gvtm_targets_apply_host(plan._h, int(voice), _ptr(offsets), _ptr(steps), _ptr(values), int(n_steps), _ptr(out),
                                                        ctypes.byref(status)))
    return out, int(status.value)


def targets_apply_host_from(plan, lists, first_step, n_steps, sums, voice=0):
    """gvtm_targets_apply_host_from: the steps [first_step, first_step + n_steps) of the utterance whose 16 lists (absolute
    steps, possibly trimmed to what the rule still needs) are `lists`, resumed on `sums` (float64 [16], the sums after step
    first_step - 1; not read at first_step 0) -> (the parameters by step float32 [n_steps][16], the sums after the last step
    float64 [16], status).  `sums` itself is left alone."""
    assert len(lists) == N_PARAM
    offsets, steps, values = pack_targets(lists)
    out = np.zeros((max(int(n_steps), 0), N_PARAM), dtype=np.float32)
    sums = np.array(sums, dtype=np.float64).reshape(N_PARAM)
    status = ctypes.c_int32(-1)
    _check(plan._lib, plan._lib.gvtm_targets_apply_host_from(plan._h, int(voice), _ptr(offsets), _ptr(steps), _ptr(values), int(first_step), int(n_steps),
                                                             _ptr(sums), _ptr(out), ctypes.byref(status)))
    return out, sums, int(status.value)


def generate_tracks_host(config, event_lists, max_frames, drift=None, device=0):
    """event_lists: list of gvtm_event record arrays -> (params float32 [B][max_frames][16], frame_counts int32 [B], drift out)."""
    lib = load_library()
    batch = len(event_lists)
    offsets = np.zeros(batch + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e) for e in event_lists])
    events = np.concatenate([np.ascontiguousarray(e, dtype=EVENT_DTYPE) for e in event_lists]) if batch else np.zeros(0, EVENT_DTYPE)
    params = np.zeros((batch, max_frames, 16), dtype=np.float32)
    counts = np.zeros(batch, dtype=np.int32)
    dr = None
    if drift is not None:
        dr = np.zeros(batch, dtype=DRIFT_DTYPE)
        for b, st in enumerate(drift):
            dr[b] = tuple(st)
    _check(lib, lib.gvtm_generate_tracks_host(int(device), ctypes.byref(config), _ptr(events), _ptr(offsets), batch, int(max_frames),
                                              _ptr(params), _ptr(counts), _ptr(dr)))
    return params, counts, dr


def generate_tracks_device(config, d_events, d_offsets, batch, max_frames, d_params, d_frame_counts=None, d_drift=None,
                           stream=None, device=0):
    lib = load_library()
    _check(lib, lib.gvtm_generate_tracks_device(int(device), ctypes.byref(config), _ptr(d_events), _ptr(d_offsets), int(batch),
                                                int(max_frames), _ptr(d_params), _ptr(d_frame_counts), _ptr(d_drift), _ptr(stream)))


def _ptr(x):
    """Device/host pointer of a torch tensor, numpy array, int or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())  # torch.Tensor


ANALYSIS_FFT_SIZE = 65536  # GVTM_ANALYSIS_FFT_SIZE
ANALYSIS_MAX_BINS = 32769  # GVTM_ANALYSIS_MAX_BINS
ANALYSIS_DEFAULT_BUFFERS = 128  # GVTM_ANALYSIS_DEFAULT_BUFFERS
WINDOW_RECTANGULAR, WINDOW_TRIANGULAR, WINDOW_HANN, WINDOW_HAMMING, WINDOW_BLACKMAN = range(5)  # GVTM_WINDOW_*


class AnalysisConfig(ctypes.Structure):
    """gvtm_analysis_config"""
    _fields_ = [("window_type", ctypes.c_int32), ("window_size", ctypes.c_int32), ("log_scale", ctypes.c_int32),
                ("min_db", ctypes.c_double), ("max_freq_hz", ctypes.c_double), ("sample_rate", ctypes.c_uint32)]


LISTEN_SPECTRA, LISTEN_SIGNAL = 1, 2  # GVTM_LISTEN_*


def listen_buffer_count(fill, n_new):
    """gvtm_listen_buffer_count -> (the buffers n_new more samples complete on a ring holding `fill`, the ring's fill afterwards)."""
    after = ctypes.c_int64(0)
    n = load_library().gvtm_listen_buffer_count(int(fill), int(n_new), ctypes.byref(after))
    return int(n), int(after.value)


def analysis_buffer_count(n_samples, first_sample, max_buffers):
    """gvtm_analysis_buffer_count: the complete buffers of 65 536 samples from first_sample on, max_buffers at the most."""
    return int(load_library().gvtm_analysis_buffer_count(int(n_samples), int(first_sample), int(max_buffers)))


class Analysis:
    """Owns a gvtm_analysis: the interactive window's spectrum and signal views of synthesized audio (include/gama_vtm.h,
    "Spectrum analysis").  device=DEVICE_NONE gives a design-only object: window, bin count and the host restatement.
    diagnostics=True binds the object to libgama_vtm_diag.so, whose gvtm_debug_* hooks the last two methods call."""

    def __init__(self, window_type=WINDOW_BLACKMAN, window_size=ANALYSIS_FFT_SIZE, log_scale=True, min_db=-120.0, max_freq_hz=0.0,
                 sample_rate=44100, device=0, diagnostics=False):
        self._lib = load_library(diagnostics)
        self._h = ctypes.c_void_p()
        self.config = AnalysisConfig(int(window_type), int(window_size), int(bool(log_scale)), float(min_db), float(max_freq_hz), int(sample_rate))
        _check(self._lib, self._lib.gvtm_analysis_create(int(device), ctypes.byref(self.config), ctypes.byref(self._h)))
        self.window_size = int(window_size)
        self.n_bins = _count(self._lib, self._lib.gvtm_analysis_bin_count(self._h))

    def close(self):
        if self._h:
            self._lib.gvtm_analysis_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def window(self):
        """The window's W doubles, as designed on the host."""
        out = np.empty(self.window_size, dtype=np.float64)
        _check(self._lib, self._lib.gvtm_analysis_window(self._h, _ptr(out), out.size))
        return out

    def reserve(self, n_buffers):
        """gvtm_analysis_reserve: device scratch for n_buffers buffers in flight (synchronous)."""
        _check(self._lib, self._lib.gvtm_analysis_reserve(self._h, int(n_buffers)))

    def apply_host(self, samples, first_sample=0, max_buffers=1, spectra=True, signal=True, fill=np.nan):
        """gvtm_analysis_apply_host on one utterance's samples -> (spectra float32 [max_buffers][n_bins] or None, signal
        float32 [max_buffers][W] or None, the number of buffers analysed); rows behind it keep `fill`."""
        samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        spec = np.full((int(max_buffers), self.n_bins), fill, dtype=np.float32) if spectra else None
        sig = np.full((int(max_buffers), self.window_size), fill, dtype=np.float32) if signal else None
        n = ctypes.c_size_t(0)
        _check(self._lib, self._lib.gvtm_analysis_apply_host(self._h, _ptr(samples), samples.size, int(first_sample), int(max_buffers), _ptr(spec),
                                                             _ptr(sig), ctypes.byref(n)))
        return spec, sig, int(n.value)

    def analyze_device(self, d_audio, audio_stride, d_counts, batch, max_buffers, d_first=None, d_spectra=None, d_signal=None,
                       d_buffers_out=None, stream=None):
        """gvtm_analyze_spectrum_device, enqueue-only: device tensors (or pointers) in the layouts the header gives."""
        _check(self._lib, self._lib.gvtm_analyze_spectrum_device(self._h, _ptr(d_audio), int(audio_stride), _ptr(d_counts), _ptr(d_first), int(batch),
                                                                 int(max_buffers), _ptr(d_spectra), _ptr(d_signal), _ptr(d_buffers_out), _ptr(stream)))

    def debug_analyze_slots(self, d_audio, audio_stride, d_counts, batch, max_buffers, d_out_slots, out_stride, d_first=None, d_spectra=None,
                            d_signal=None, d_buffers_out=None, stream=None):
        """gvtm_debug_analyze_slots (diagnostics): analyze_device with utterance b's buffers at the rows d_out_slots[b] + k of its
        block of out_stride rows of the outputs."""
        _check(self._lib, self._lib.gvtm_debug_analyze_slots(self._h, _ptr(d_audio), int(audio_stride), _ptr(d_counts), _ptr(d_first), int(batch),
                                                             int(max_buffers), _ptr(d_spectra), _ptr(d_signal), _ptr(d_buffers_out), _ptr(d_out_slots),
                                                             int(out_stride), _ptr(stream)))

    def debug_float_host(self, samples):
        """gvtm_debug_analysis_float_host (diagnostics): the linear spectrum [n_bins] of one buffer of 65 536 samples by the
        float transform of csrc/vtm_analysis.hpp run on the host."""
        samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        assert samples.size == ANALYSIS_FFT_SIZE, samples.size
        out = np.full(self.n_bins, np.nan, dtype=np.float32)
        _check(self._lib, self._lib.gvtm_debug_analysis_float_host(self._h, _ptr(samples), _ptr(out)))
        return out


def debug_listen_move(fill, n):
    """gvtm_debug_listen_move (diagnostics): listen_move(fill, n) of csrc/vtm_listen.hpp as a dict of its six fields."""
    out = np.zeros(6, dtype=np.int64)
    lib = load_library(True)
    _check(lib, lib.gvtm_debug_listen_move(int(fill), int(n), _ptr(out)))
    return dict(zip(("buffers", "fill_after", "head_len", "inside_first", "tail_src", "tail_len"), (int(v) for v in out)))


def debug_listen_copy(d_src, src_stride, d_dst, dst_stride, d_src_off, d_dst_off, d_len, batch, max_len, device=0):
    """gvtm_debug_listen_copy (diagnostics): the ragged copy of a listening stream alone on device tensors (or pointers),
    synchronous."""
    lib = load_library(True)
    _check(lib, lib.gvtm_debug_listen_copy(int(device), _ptr(d_src), int(src_stride), _ptr(d_dst), int(dst_stride), _ptr(d_src_off), _ptr(d_dst_off),
                                           _ptr(d_len), int(batch), int(max_len)))


_NO_VOICE_IDS = object()  # (Plan._synthesize_targets: the entry has no d_voice_ids argument)


class Plan:
    """Owns a gvtm_plan.  device=DEVICE_NONE gives a design-only plan (no GPU needed)."""

    def __init__(self, config, control_rate=250.0, device=0, diagnostics=False, rows=0, float_model5=False):
        """diagnostics=True binds the plan to libgama_vtm_diag.so (gvtm_debug_* hooks); rows (diagnostics only) forces
        the utterances per workgroup, i.e. the kernel shape a big batch would get.  float_model5=True (a Config5 with
        precision PRECISION_F32) makes the plan of VocalTractModel5<float,1> through gvtm_plan_create_model5_float."""
        self._open(diagnostics)
        self.config = config
        create = self._lib.gvtm_plan_create_model5 if isinstance(config, Config5) else self._lib.gvtm_plan_create
        if float_model5:
            if not isinstance(config, Config5):
                raise ValueError("float_model5 needs a Config5")
            create = self._lib.gvtm_plan_create_model5_float
        self._created(create(ctypes.byref(config), float(control_rate), int(device), ctypes.byref(self._h)), rows)

    def _open(self, diagnostics):
        self._lib = load_library(diagnostics)
        self.diagnostics = bool(diagnostics)
        self._h = ctypes.c_void_p()

    def _created(self, rc, rows):
        """What follows gvtm_plan_create* for every plan: its status, the plan's info (voice 0's) and the forced rows."""
        self._check(rc)
        self.info = Info()
        self._check(self._lib.gvtm_plan_info(self._h, ctypes.byref(self.info)))
        if rows:
            if not self.diagnostics:
                raise ValueError("rows can only be forced on a diagnostics plan")
            self._check(self._lib.gvtm_debug_set_rows(self._h, int(rows)))

    def _check(self, rc):
        if rc != 0:
            _check(self._lib, rc)

    def close(self):
        if self._h:
            self._lib.gvtm_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def table(self, which):
        buf = np.empty(4096, dtype=np.float64)
        n = self._lib.gvtm_plan_table(self._h, which, buf.ctypes.data, buf.size)
        if n < 0:
            self._check(-n)
        return buf[:n].copy()

    def uses_fir_literals(self):
        """Diagnostics plans: whether launches take the float decimator's coefficients from the kernels' literal table."""
        rc = self._lib.gvtm_debug_plan_fir_literals(self._h)
        if rc < 0:
            self._check(-rc)
        return bool(rc)

    def force_generic_fir(self):
        """Diagnostics plans: later launches run the generic tap loop over the plan's own coefficients."""
        self._check(self._lib.gvtm_debug_force_generic_fir(self._h))

    def _hook_count(self, rc):
        if rc < 0:
            self._check(-rc)
        return int(rc)

    def src_phases(self):
        """Diagnostics plans: the output phases of the plan's table of converter coefficients, 0 for a plan without one."""
        return self._hook_count(self._lib.gvtm_debug_plan_src_phases(self._h))

    def src_phase_table(self):
        """Diagnostics plans: that table as the host designs it, float32 [phases][28]; None for a plan without one."""
        phases = self.src_phases()
        if not phases:
            return None
        out = np.empty((phases, 28), dtype=np.float32)
        assert self._hook_count(self._lib.gvtm_debug_plan_src_phase_table(self._h, out.ctypes.data, out.size)) == phases
        return out

    def force_generic_src(self):
        """Diagnostics plans: later launches form the converter's coefficients in the kernel."""
        self._check(self._lib.gvtm_debug_force_generic_src(self._h))

    def says_static_wavetable(self):
        """Diagnostics plans: whether the plan tells its launches that the wavetable never follows the amplitude."""
        return bool(self._hook_count(self._lib.gvtm_debug_plan_static_wavetable(self._h)))

    def force_dynamic_wavetable(self):
        """Diagnostics plans: later launches ask per wavetable entry whether it follows the amplitude."""
        self._check(self._lib.gvtm_debug_force_dynamic_wavetable(self._h))

    def filter_split(self, rows):
        """Diagnostics plans: which serial filter stages the kernel shape of `rows` utterances per workgroup runs with their
        feed-forward half 64 steps at a time (bit 0: the post-tube filters); 0: none."""
        return self._hook_count(self._lib.gvtm_debug_plan_filter_split(self._h, int(rows)))

    def output_count(self, frames):
        return int(self._lib.gvtm_output_count(self._h, int(frames)))

    def output_capacity(self, max_frames):
        """Row length that holds every utterance of a ragged batch (> output_count(max_frames) on down-sampling plans)."""
        return int(self._lib.gvtm_output_capacity(self._h, int(max_frames)))

    def set_timing(self, enabled):
        self._check(self._lib.gvtm_plan_set_timing(self._h, int(bool(enabled))))

    def take_kernel_ms(self):
        n = ctypes.c_int(0)
        ms = self._lib.gvtm_plan_take_kernel_ms(self._h, ctypes.byref(n))
        return float(ms), int(n.value)

    def synthesize_device(self, d_params, batch, max_frames, d_audio, audio_stride, d_frame_counts=None,
                          d_out_counts=None, d_maxabs=None, stream=None):
        """All arguments are device pointers (torch CUDA tensors or raw ints)."""
        self._check(self._lib.gvtm_synthesize_batch_device(
            self._h, _ptr(d_params), _ptr(d_frame_counts), int(batch), int(max_frames), _ptr(d_audio),
            int(audio_stride), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(stream)))

    @staticmethod
    def _host_outputs(batch, shape, dtype):
        """The arrays a host entry fills: (samples of dtype, [batch][stride] or packed [capacity]; counts int64 [batch]; maxabs
        float32 [batch]; scales float32 [batch] with int16 samples, else None)."""
        return (np.zeros(shape, dtype=dtype), np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.float32),
                np.zeros(batch, dtype=np.float32) if dtype == np.int16 else None)

    def _host(self, params, frame_counts, dtype):
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.ndim == 3 and params.shape[2] == N_PARAM
        batch, frames = params.shape[:2]
        assert frame_counts is None or np.shape(frame_counts) == (batch,)
        stride = self.output_count(frames) if frame_counts is None else self.output_capacity(frames)
        out, counts, maxabs, scales = self._host_outputs(batch, (batch, stride), dtype)
        self.synthesize_host_into(params, out, frame_counts, counts, maxabs, scales)
        return out, counts, maxabs, scales

    def synthesize_host(self, params, frame_counts=None):
        """params: float32 [B][F][16] numpy -> (audio float32 [B][stride], counts int64 [B], maxabs float32 [B])."""
        return self._host(params, frame_counts, np.float32)[:3]

    def synthesize_host_pcm16(self, params, frame_counts=None):
        """-> (pcm int16 [B][stride], counts int64 [B], maxabs float32 [B], scales float32 [B])"""
        return self._host(params, frame_counts, np.int16)

    def synthesize_host_into(self, params, out, frame_counts=None, counts=None, maxabs=None, scales=None):
        """The host entries with caller-owned (e.g. page-locked) buffers: `out` float32 [B][stride] takes the unscaled
        samples (gvtm_synthesize_batch_host), `out` int16 [B][stride] the scaled 16-bit ones (.._host_pcm16)."""
        assert params.dtype == np.float32 and params.flags.c_contiguous and params.ndim == 3 and params.shape[2] == N_PARAM
        assert out.flags.c_contiguous and out.ndim == 2 and out.shape[0] == params.shape[0]
        batch, frames = params.shape[:2]
        fc = None
        if frame_counts is not None:
            fc = np.ascontiguousarray(frame_counts, dtype=np.int32)
        if out.dtype == np.int16:
            self._check(self._lib.gvtm_synthesize_batch_host_pcm16(
                self._h, _ptr(params), _ptr(fc), batch, frames, _ptr(out), out.shape[1], _ptr(counts), _ptr(maxabs), _ptr(scales)))
        else:
            assert out.dtype == np.float32 and scales is None
            self._check(self._lib.gvtm_synthesize_batch_host(
                self._h, _ptr(params), _ptr(fc), batch, frames, _ptr(out), out.shape[1], _ptr(counts), _ptr(maxabs)))

    # ---- ragged batches, packed in and packed out (a VoicesPlan has them too; voice_ids: one per utterance) ----

    @staticmethod
    def pack_utterances(utterances):
        """A list of float32 [F_b][16] arrays -> (frames float32 [sum F_b][16] back to back, frame_offsets int64 [B + 1])."""
        utterances = [np.ascontiguousarray(u, dtype=np.float32).reshape(-1, N_PARAM) for u in utterances]
        offsets = np.zeros(len(utterances) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([u.shape[0] for u in utterances])
        frames = np.concatenate(utterances) if utterances else np.zeros((0, N_PARAM), np.float32)
        return np.ascontiguousarray(frames), offsets

    def _ids(self, voice_ids, batch):
        if voice_ids is None:
            return None
        ids = np.ascontiguousarray(voice_ids, dtype=np.int32)
        assert ids.shape == (batch,)
        return ids

    def packed_sample_offsets(self, frame_offsets, voice_ids=None):
        """gvtm_packed_sample_offsets -> int64 [B + 1]: utterance b starts at [b], the output needs [B] samples."""
        frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        batch = frame_offsets.shape[0] - 1
        out = np.zeros(batch + 1, dtype=np.int64)
        _count(self._lib, self._lib.gvtm_packed_sample_offsets(self._h, _ptr(frame_offsets), _ptr(self._ids(voice_ids, batch)), batch, _ptr(out)))
        return out

    def synthesize_packed_host_into(self, frames, frame_offsets, out, voice_ids=None, sample_offsets=None, counts=None, maxabs=None,
                                    scales=None):
        """The packed entries with caller-owned (e.g. page-locked) buffers: frames float32 [sum F_b][16], frame_offsets int64
        [B + 1]; `out` float32 [capacity] takes the unscaled samples (gvtm_synthesize_packed_host), `out` int16 [capacity] the
        scaled 16-bit ones (.._pcm16); sample_offsets int64 [B + 1], counts int64 [B], maxabs and scales float32 [B] or None."""
        assert frames.dtype == np.float32 and frames.flags.c_contiguous
        assert frame_offsets.dtype == np.int64 and frame_offsets.flags.c_contiguous and out.flags.c_contiguous and out.ndim == 1
        batch = frame_offsets.shape[0] - 1
        ids = self._ids(voice_ids, batch)
        if out.dtype == np.int16:
            self._check(self._lib.gvtm_synthesize_packed_host_pcm16(
                self._h, _ptr(frames), _ptr(frame_offsets), _ptr(ids), batch, _ptr(out), out.shape[0], _ptr(sample_offsets),
                _ptr(counts), _ptr(maxabs), _ptr(scales)))
        else:
            assert out.dtype == np.float32 and scales is None
            self._check(self._lib.gvtm_synthesize_packed_host(
                self._h, _ptr(frames), _ptr(frame_offsets), _ptr(ids), batch, _ptr(out), out.shape[0], _ptr(sample_offsets),
                _ptr(counts), _ptr(maxabs)))

    def _packed(self, utterances, voice_ids, dtype):
        frames, frame_offsets = self.pack_utterances(utterances)
        batch = len(utterances)
        offsets = self.packed_sample_offsets(frame_offsets, voice_ids)
        out, counts, maxabs, scales = self._host_outputs(batch, int(offsets[batch]), dtype)
        self.synthesize_packed_host_into(frames, frame_offsets, out, voice_ids, offsets, counts, maxabs, scales)
        return out, offsets, counts, maxabs, scales

    def synthesize_packed_host(self, utterances, voice_ids=None):
        """utterances: a list of float32 [F_b][16] arrays -> (audio float32 [capacity], sample offsets int64 [B + 1], counts
        int64 [B], maxabs float32 [B]); utterance b's samples are audio[offsets[b]: offsets[b] + counts[b]]."""
        return self._packed(utterances, voice_ids, np.float32)[:4]

    def synthesize_packed_host_pcm16(self, utterances, voice_ids=None):
        """-> (pcm int16 [capacity], sample offsets, counts, maxabs, scales float32 [B])"""
        return self._packed(utterances, voice_ids, np.int16)

    def set_staging_limit(self, nbytes):
        """gvtm_plan_set_staging_limit: an upper bound on the packed entries' device staging; 0 = none."""
        self._check(self._lib.gvtm_plan_set_staging_limit(self._h, int(nbytes)))

    def packed_stats(self):
        st = PackedStats()
        self._check(self._lib.gvtm_plan_packed_stats(self._h, ctypes.byref(st)))
        return st

    def reserve(self, max_frames):
        """gvtm_plan_reserve: what launches of up to max_frames frames would build on first use, now."""
        self._check(self._lib.gvtm_plan_reserve(self._h, int(max_frames)))

    # ---- event lists in from host memory, packed samples out (a VoicesPlan has them too) ----

    def set_voice_tracks(self, configs):
        """gvtm_plan_set_voice_tracks: configs[v] is the TrackConfig of voice v (one per voice of the plan)."""
        configs = list(configs)
        arr = (TrackConfig * max(len(configs), 1))(*configs)
        self._check(self._lib.gvtm_plan_set_voice_tracks(self._h, arr, len(configs)))

    @staticmethod
    def pack_event_lists(utterances):
        """utterances[b]: the event tables (float64 [E][38] rows, events_from_table) of utterance b's chunks -> (gvtm_event
        records of every chunk back to back, chunk_offsets int64 [chunks + 1], utt_chunks int64 [B + 1])."""
        chunks = [np.ascontiguousarray(events_from_table(t)) for u in utterances for t in u]
        chunk_offsets = np.zeros(len(chunks) + 1, dtype=np.int64)
        chunk_offsets[1:] = np.cumsum([len(c) for c in chunks])
        utt_chunks = np.zeros(len(utterances) + 1, dtype=np.int64)
        utt_chunks[1:] = np.cumsum([len(u) for u in utterances])
        events = np.concatenate(chunks) if chunks else np.zeros(0, dtype=EVENT_DTYPE)
        return np.ascontiguousarray(events), chunk_offsets, utt_chunks

    def events_packed_layout(self, events, chunk_offsets, utt_chunks, voice_ids=None):
        """gvtm_events_packed_layout -> (frame offsets int64 [B + 1], sample offsets int64 [B + 1]): utterance b yields
        frame_offsets[b + 1] - frame_offsets[b] frames and starts at sample_offsets[b]; the output needs sample_offsets[B]
        samples."""
        assert events.dtype == EVENT_DTYPE and events.flags.c_contiguous
        chunk_offsets = np.ascontiguousarray(chunk_offsets, dtype=np.int64)
        utt_chunks = np.ascontiguousarray(utt_chunks, dtype=np.int64)
        batch = utt_chunks.shape[0] - 1
        frame_offsets, sample_offsets = np.zeros(batch + 1, dtype=np.int64), np.zeros(batch + 1, dtype=np.int64)
        _count(self._lib, self._lib.gvtm_events_packed_layout(self._h, _ptr(events), _ptr(chunk_offsets), _ptr(utt_chunks),
                                                              _ptr(self._ids(voice_ids, batch)), batch, _ptr(frame_offsets), _ptr(sample_offsets)))
        return frame_offsets, sample_offsets

    def synthesize_events_packed_host_into(self, events, chunk_offsets, utt_chunks, out, voice_ids=None, sample_offsets=None,
                                           frame_offsets=None, frames_out=None, counts=None, maxabs=None, scales=None, drift=None):
        """The events-packed entries with caller-owned (e.g. page-locked) buffers: gvtm_event records, chunk_offsets int64
        [chunks + 1], utt_chunks int64 [B + 1]; `out` float32 [capacity] takes the unscaled samples
        (gvtm_synthesize_events_packed_host), `out` int16 [capacity] the scaled 16-bit ones (.._pcm16); sample_offsets and
        frame_offsets int64 [B + 1], frames_out float32 [frames][16], counts int64 [B], maxabs and scales float32 [B], drift
        float64 [B][5] in/out, or None."""
        assert events.dtype == EVENT_DTYPE and events.flags.c_contiguous
        assert chunk_offsets.dtype == np.int64 and chunk_offsets.flags.c_contiguous
        assert utt_chunks.dtype == np.int64 and utt_chunks.flags.c_contiguous and out.flags.c_contiguous and out.ndim == 1
        batch = utt_chunks.shape[0] - 1
        ids = self._ids(voice_ids, batch)
        frames_capacity = 0
        if frames_out is not None:
            assert frames_out.dtype == np.float32 and frames_out.flags.c_contiguous and frames_out.shape[-1] == N_PARAM
            frames_capacity = frames_out.size // N_PARAM
        if drift is not None:
            assert drift.dtype == np.float64 and drift.flags.c_contiguous and drift.shape == (batch, 5)
        if out.dtype == np.int16:
            self._check(self._lib.gvtm_synthesize_events_packed_host_pcm16(
                self._h, _ptr(events), _ptr(chunk_offsets), _ptr(utt_chunks), _ptr(ids), batch, _ptr(out), out.shape[0], _ptr(sample_offsets),
                _ptr(frame_offsets), _ptr(frames_out), frames_capacity, _ptr(counts), _ptr(maxabs), _ptr(scales), _ptr(drift)))
        else:
            assert out.dtype == np.float32 and scales is None
            self._check(self._lib.gvtm_synthesize_events_packed_host(
                self._h, _ptr(events), _ptr(chunk_offsets), _ptr(utt_chunks), _ptr(ids), batch, _ptr(out), out.shape[0], _ptr(sample_offsets),
                _ptr(frame_offsets), _ptr(frames_out), frames_capacity, _ptr(counts), _ptr(maxabs), _ptr(drift)))

    def apply_intonation_device(self, d_events, d_list_offsets, n_lists, d_list_ids, d_points, d_point_offsets, d_voice_ids, batch,
                                d_events_out, out_capacity, d_event_offsets_out, d_status=None, stream=None):
        """gvtm_apply_intonation_device: intonation points onto base event lists (d_list_ids None: utterance b's is list
        b) -> merged lists, their offsets and statuses; all pointers are device memory."""
        self._check(self._lib.gvtm_apply_intonation_device(
            self._h, _ptr(d_events), _ptr(d_list_offsets), int(n_lists), _ptr(d_list_ids), _ptr(d_points), _ptr(d_point_offsets),
            _ptr(d_voice_ids), int(batch), _ptr(d_events_out), int(out_capacity), _ptr(d_event_offsets_out), _ptr(d_status), _ptr(stream)))

    def synthesize_intonation_device(self, d_events, d_list_offsets, n_lists, d_list_ids, d_points, d_point_offsets, d_voice_ids,
                                     events_capacity, batch, max_frames, d_audio, audio_stride, d_frame_counts=None, d_out_counts=None,
                                     d_maxabs=None, d_drift=None, d_status=None, stream=None):
        """Base event lists and intonation points in, samples out (gvtm_synthesize_intonation_device); all pointers are
        device memory."""
        self._check(self._lib.gvtm_synthesize_intonation_device(
            self._h, _ptr(d_events), _ptr(d_list_offsets), int(n_lists), _ptr(d_list_ids), _ptr(d_points), _ptr(d_point_offsets),
            _ptr(d_voice_ids), int(events_capacity), int(batch), int(max_frames), _ptr(d_audio), int(audio_stride), _ptr(d_frame_counts),
            _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_drift), _ptr(d_status), _ptr(stream)))

    def modification_filter_length(self, voice=0):
        """gvtm_modification_filter_length: the samples of the 20 ms moving average at the voice's internal rate."""
        n = int(self._lib.gvtm_modification_filter_length(self._h, int(voice)))
        if n < 0:
            raise GvtmError(1, self._lib.gvtm_last_error().decode())
        return n

    def apply_modifications_device(self, d_base_params, d_base_frame_counts, n_bases, d_base_ids, d_gestures, d_gesture_offsets, d_utt_gestures,
                                   d_point_steps, d_point_values, d_voice_ids, batch, max_frames, d_params_out, d_frame_counts_out,
                                   d_status=None, stream=None):
        """gvtm_apply_modifications_device: gestures (the tables of pack_gestures) onto base frames (d_base_ids None:
        utterance b's is base b; d_voice_ids None: the plan's one voice) -> modified frames, frame counts and statuses; all
        pointers are device memory."""
        self._check(self._lib.gvtm_apply_modifications_device(
            self._h, _ptr(d_base_params), _ptr(d_base_frame_counts), int(n_bases), _ptr(d_base_ids), _ptr(d_gestures), _ptr(d_gesture_offsets),
            _ptr(d_utt_gestures), _ptr(d_point_steps), _ptr(d_point_values), _ptr(d_voice_ids), int(batch), int(max_frames), _ptr(d_params_out),
            _ptr(d_frame_counts_out), _ptr(d_status), _ptr(stream)))

    def synthesize_modified_device(self, d_base_params, d_base_frame_counts, n_bases, d_base_ids, d_gestures, d_gesture_offsets, d_utt_gestures,
                                   d_point_steps, d_point_values, d_voice_ids, batch, max_frames, d_audio, audio_stride, d_frame_counts=None,
                                   d_out_counts=None, d_maxabs=None, d_status=None, stream=None):
        """Base frames and gestures in, samples out (gvtm_synthesize_modified_device); all pointers are device memory."""
        self._check(self._lib.gvtm_synthesize_modified_device(
            self._h, _ptr(d_base_params), _ptr(d_base_frame_counts), int(n_bases), _ptr(d_base_ids), _ptr(d_gestures), _ptr(d_gesture_offsets),
            _ptr(d_utt_gestures), _ptr(d_point_steps), _ptr(d_point_values), _ptr(d_voice_ids), int(batch), int(max_frames), _ptr(d_audio),
            int(audio_stride), _ptr(d_frame_counts), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_status), _ptr(stream)))

    def targets_filter_length(self, voice=0):
        """gvtm_targets_filter_length: the samples of the interactive window's 50 ms moving average at the voice's internal rate."""
        n = int(self._lib.gvtm_targets_filter_length(self._h, int(voice)))
        if n < 0:
            raise GvtmError(1, self._lib.gvtm_last_error().decode())
        return n

    def targets_output_count(self, steps):
        """gvtm_targets_output_count: the samples of an utterance of `steps` internal steps."""
        return _count(self._lib, int(self._lib.gvtm_targets_output_count(self._h, int(steps))))

    def targets_output_capacity(self, max_steps):
        """gvtm_targets_output_capacity: the row length that holds every utterance of up to max_steps steps."""
        return _count(self._lib, int(self._lib.gvtm_targets_output_capacity(self._h, int(max_steps))))

    def synthesize_targets_device(self, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, batch, max_steps,
                                  d_audio, audio_stride, d_out_counts=None, d_maxabs=None, d_status=None, stream=None):
        """Target lists (the tables of pack_targets; d_list_ids None: utterance b's parameter p walks list 16 b + p) in,
        samples out (gvtm_synthesize_targets_device); all pointers are device memory."""
        self._synthesize_targets(self._lib.gvtm_synthesize_targets_device, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values,
                                 d_step_counts, batch, max_steps, d_audio, audio_stride, d_out_counts, d_maxabs, d_status, stream)

    def _synthesize_targets(self, entry, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, batch, max_steps, d_audio,
                            audio_stride, d_out_counts, d_maxabs, d_status, stream, d_voice_ids=_NO_VOICE_IDS):
        """What the four synthesize_targets*_device methods do: `entry`, with d_voice_ids where the entry takes them (None is NULL there)."""
        voices = () if d_voice_ids is _NO_VOICE_IDS else (_ptr(d_voice_ids),)
        self._check(entry(self._h, _ptr(d_list_offsets), int(n_lists), _ptr(d_list_ids), _ptr(d_point_steps), _ptr(d_point_values), _ptr(d_step_counts),
                          *voices, int(batch), int(max_steps), _ptr(d_audio), int(audio_stride), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_status),
                          _ptr(stream)))

    def synthesize_targets_model5_device(self, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, batch, max_steps,
                                         d_audio, audio_stride, d_out_counts=None, d_maxabs=None, d_status=None, stream=None):
        """synthesize_targets_device for a one-voice model 5 plan of either class (gvtm_synthesize_targets_model5_device): the
        samples of the model as the interactive window constructs it, each step's signal divided by its f0.  All pointers are
        device memory."""
        self._synthesize_targets(self._lib.gvtm_synthesize_targets_model5_device, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values,
                                 d_step_counts, batch, max_steps, d_audio, audio_stride, d_out_counts, d_maxabs, d_status, stream)

    def targets_voice_output_count(self, voice, steps):
        """gvtm_targets_voice_output_count: the samples of an utterance of `steps` internal steps under voice `voice`;
        (size_t)-1 for a voice outside the plan's, as voice_output_count."""
        return int(self._lib.gvtm_targets_voice_output_count(self._h, int(voice), int(steps)))

    def targets_voices_output_capacity(self, max_steps):
        """gvtm_targets_voices_output_capacity: the row length that holds every utterance of up to max_steps steps under any voice."""
        return int(self._lib.gvtm_targets_voices_output_capacity(self._h, int(max_steps)))

    def synthesize_targets_voices_device(self, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, d_voice_ids,
                                         batch, max_steps, d_audio, audio_stride, d_out_counts=None, d_maxabs=None, d_status=None, stream=None):
        """synthesize_targets_device with a voice id per utterance (gvtm_synthesize_targets_voices_device): utterance b walks
        its lists under voice d_voice_ids[b]; on a plan of one voice the ids are all 0.  All pointers are device memory."""
        self._synthesize_targets(self._lib.gvtm_synthesize_targets_voices_device, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values,
                                 d_step_counts, batch, max_steps, d_audio, audio_stride, d_out_counts, d_maxabs, d_status, stream, d_voice_ids)

    def synthesize_targets_model5_voices_device(self, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values, d_step_counts, d_voice_ids,
                                                batch, max_steps, d_audio, audio_stride, d_out_counts=None, d_maxabs=None, d_status=None, stream=None):
        """synthesize_targets_model5_device with a voice id per utterance (gvtm_synthesize_targets_model5_voices_device), for
        model 5 voices plans of either class: utterance b walks its lists under voice d_voice_ids[b], its samples the
        interactive model's; on a plan of one voice the ids are all 0.  All pointers are device memory."""
        self._synthesize_targets(self._lib.gvtm_synthesize_targets_model5_voices_device, d_list_offsets, n_lists, d_list_ids, d_point_steps, d_point_values,
                                 d_step_counts, batch, max_steps, d_audio, audio_stride, d_out_counts, d_maxabs, d_status, stream, d_voice_ids)

    def synthesize_events_device(self, track_config, d_events, d_offsets, batch, max_frames, d_audio, audio_stride,
                                 d_frame_counts=None, d_out_counts=None, d_maxabs=None, d_drift=None, stream=None):
        """Event lists in, samples out, one launch (gvtm_synthesize_events_device); all pointers are device memory."""
        self._check(self._lib.gvtm_synthesize_events_device(
            self._h, ctypes.byref(track_config), _ptr(d_events), _ptr(d_offsets), int(batch), int(max_frames), _ptr(d_audio),
            int(audio_stride), _ptr(d_frame_counts), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_drift), _ptr(stream)))

    def synthesize_postures_device(self, rules, track_config, d_postures, d_posture_offsets, events_capacity, batch, max_frames, d_audio,
                                   audio_stride, d_frame_counts=None, d_out_counts=None, d_maxabs=None, d_drift=None, d_status=None, stream=None):
        """Posture sequences in, samples out (gvtm_synthesize_postures_device; rules: a Rules on the plan's device); all
        pointers are device memory."""
        self._check(self._lib.gvtm_synthesize_postures_device(
            self._h, rules._h, ctypes.byref(track_config), _ptr(d_postures), _ptr(d_posture_offsets), int(events_capacity), int(batch),
            int(max_frames), _ptr(d_audio), int(audio_stride), _ptr(d_frame_counts), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_drift),
            _ptr(d_status), _ptr(stream)))

    def synthesize_prosody_device(self, rules, prosody, d_postures, d_posture_offsets, n_postures, d_feet, d_foot_offsets, n_feet, d_groups, d_group_offsets,
                                  d_draws, d_voice_ids, max_rules, points_capacity, events_capacity, batch, max_frames, d_audio, audio_stride,
                                  d_frame_counts=None, d_out_counts=None, d_maxabs=None, d_drift=None, d_prosody_status=None, d_status=None, stream=None):
        """Postures, feet and tone groups in, samples out (gvtm_synthesize_prosody_device; a plan with track configurations,
        rules and prosody on its device); all pointers are device memory, everything is enqueued on `stream`."""
        self._check(self._lib.gvtm_synthesize_prosody_device(
            self._h, rules._h, prosody._h, _ptr(d_postures), _ptr(d_posture_offsets), int(n_postures), _ptr(d_feet), _ptr(d_foot_offsets), int(n_feet),
            _ptr(d_groups), _ptr(d_group_offsets), _ptr(d_draws), _ptr(d_voice_ids), int(max_rules), int(points_capacity), int(events_capacity), int(batch),
            int(max_frames), _ptr(d_audio), int(audio_stride), _ptr(d_frame_counts), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_drift), _ptr(d_prosody_status),
            _ptr(d_status), _ptr(stream)))

    def normalize_device(self, d_audio, batch, audio_stride, d_maxabs, d_counts=None, d_out_f32=None, d_out_i16=None,
                         d_scales=None, stream=None):
        self._check(self._lib.gvtm_normalize_batch_device(
            self._h, _ptr(d_audio), int(batch), int(audio_stride), _ptr(d_counts), _ptr(d_maxabs), _ptr(d_out_f32),
            _ptr(d_out_i16), _ptr(d_scales), _ptr(stream)))


class VoicesPlan(Plan):
    """Owns a gvtm_plan of several voices: configs[v] is voice v, all Config (gvtm_plan_create_voices) or all Config5
    (gvtm_plan_create_model5_voices; with float_model5=True, and precision PRECISION_F32 in every Config5, the float class
    through gvtm_plan_create_model5_float_voices).  Its batches mix voices, one voice id per utterance; the single-voice
    entries (Plan.synthesize_*, Stream) are refused on it when it has two or more."""

    def __init__(self, configs, control_rate=250.0, device=0, diagnostics=False, rows=0, float_model5=False):
        self._open(diagnostics)
        self.configs = list(configs)
        self.config = self.configs[0] if self.configs else None
        model5 = isinstance(self.config, Config5)
        if any(isinstance(c, Config5) != model5 for c in self.configs):
            raise TypeError("a plan's voices are all Config or all Config5")
        if float_model5 and not model5:
            raise ValueError("float_model5 needs Config5 voices")
        create5 = "gvtm_plan_create_model5_float_voices" if float_model5 else "gvtm_plan_create_model5_voices"
        ctype, create = (Config5, getattr(self._lib, create5)) if model5 else (Config, self._lib.gvtm_plan_create_voices)
        arr = (ctype * max(len(self.configs), 1))(*self.configs)
        self._created(create(arr, len(self.configs), float(control_rate), int(device), ctypes.byref(self._h)), rows)
        self.n_voices = int(self._lib.gvtm_plan_voice_count(self._h))

    def voice_info(self, voice):
        info = Info()
        self._check(self._lib.gvtm_plan_voice_info(self._h, int(voice), ctypes.byref(info)))
        return info

    def voice_output_count(self, voice, frames):
        return int(self._lib.gvtm_voice_output_count(self._h, int(voice), int(frames)))

    def voices_output_capacity(self, max_frames):
        """Row length that holds every utterance of any mix of voices (ragged frame counts included)."""
        return int(self._lib.gvtm_voices_output_capacity(self._h, int(max_frames)))

    def synthesize_voices_device(self, d_params, d_voice_ids, batch, max_frames, d_audio, audio_stride, d_frame_counts=None,
                                 d_out_counts=None, d_maxabs=None, stream=None):
        """gvtm_synthesize_voices_device; all arguments are device pointers (torch tensors or raw ints)."""
        self._check(self._lib.gvtm_synthesize_voices_device(
            self._h, _ptr(d_params), _ptr(d_frame_counts), _ptr(d_voice_ids), int(max_frames), int(batch), _ptr(d_audio),
            int(audio_stride), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(stream)))

    def generate_tracks_voices_device(self, d_events, d_offsets, d_voice_ids, batch, max_frames, d_params, d_frame_counts=None,
                                      d_drift=None, stream=None):
        """gvtm_generate_tracks_voices_device; all pointers are device memory."""
        self._check(self._lib.gvtm_generate_tracks_voices_device(
            self._h, _ptr(d_events), _ptr(d_offsets), _ptr(d_voice_ids), int(batch), int(max_frames), _ptr(d_params),
            _ptr(d_frame_counts), _ptr(d_drift), _ptr(stream)))

    def synthesize_events_voices_device(self, d_events, d_offsets, d_voice_ids, batch, max_frames, d_audio, audio_stride,
                                        d_frame_counts=None, d_out_counts=None, d_maxabs=None, d_drift=None, stream=None):
        """Event lists of a mix of voices in, samples out (gvtm_synthesize_events_voices_device); all pointers are device
        memory."""
        self._check(self._lib.gvtm_synthesize_events_voices_device(
            self._h, _ptr(d_events), _ptr(d_offsets), _ptr(d_voice_ids), int(batch), int(max_frames), _ptr(d_audio),
            int(audio_stride), _ptr(d_frame_counts), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_drift), _ptr(stream)))

    def generate_tracks_chunks_device(self, d_events, d_chunk_offsets, d_utt_chunks, d_voice_ids, batch, max_frames, d_params,
                                      d_frame_counts=None, d_drift=None, stream=None):
        """gvtm_generate_tracks_chunks_device: utterances of several event lists; all pointers are device memory."""
        self._check(self._lib.gvtm_generate_tracks_chunks_device(
            self._h, _ptr(d_events), _ptr(d_chunk_offsets), _ptr(d_utt_chunks), _ptr(d_voice_ids), int(batch), int(max_frames),
            _ptr(d_params), _ptr(d_frame_counts), _ptr(d_drift), _ptr(stream)))

    def synthesize_events_chunks_device(self, d_events, d_chunk_offsets, d_utt_chunks, d_voice_ids, batch, max_frames, d_audio,
                                        audio_stride, d_frame_counts=None, d_out_counts=None, d_maxabs=None, d_drift=None, stream=None):
        """Utterances of several event lists in, samples out (gvtm_synthesize_events_chunks_device); all pointers are device
        memory."""
        self._check(self._lib.gvtm_synthesize_events_chunks_device(
            self._h, _ptr(d_events), _ptr(d_chunk_offsets), _ptr(d_utt_chunks), _ptr(d_voice_ids), int(batch), int(max_frames),
            _ptr(d_audio), int(audio_stride), _ptr(d_frame_counts), _ptr(d_out_counts), _ptr(d_maxabs), _ptr(d_drift), _ptr(stream)))

    def _voices_host(self, params, voice_ids, frame_counts, dtype):
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.ndim == 3 and params.shape[2] == N_PARAM
        batch, frames = params.shape[:2]
        ids = np.ascontiguousarray(voice_ids, dtype=np.int32)
        assert ids.shape == (batch,)
        fc = None
        if frame_counts is not None:
            fc = np.ascontiguousarray(frame_counts, dtype=np.int32)
            assert fc.shape == (batch,)
        stride = self.voices_output_capacity(frames)
        out, counts, maxabs, scales = self._host_outputs(batch, (batch, stride), dtype)
        if scales is None:
            self._check(self._lib.gvtm_synthesize_voices_host(
                self._h, _ptr(params), _ptr(fc), _ptr(ids), frames, batch, _ptr(out), stride, _ptr(counts), _ptr(maxabs)))
        else:
            self._check(self._lib.gvtm_synthesize_voices_host_pcm16(
                self._h, _ptr(params), _ptr(fc), _ptr(ids), frames, batch, _ptr(out), stride, _ptr(counts), _ptr(maxabs), _ptr(scales)))
        return out, counts, maxabs, scales

    def synthesize_host(self, params, voice_ids, frame_counts=None):
        """params float32 [B][F][16], voice_ids int [B] -> (audio float32 [B][stride], counts int64 [B], maxabs float32 [B]);
        stride = voices_output_capacity(F), rows zero beyond their count."""
        return self._voices_host(params, voice_ids, frame_counts, np.float32)[:3]

    def synthesize_host_pcm16(self, params, voice_ids, frame_counts=None):
        """-> (pcm int16 [B][stride], counts int64 [B], maxabs float32 [B], scales float32 [B])"""
        return self._voices_host(params, voice_ids, frame_counts, np.int16)


class Stream:
    """Owns a gvtm_stream: `batch` utterances of a plan synthesized piece by piece (include/gama_vtm.h, "Streams").
    With voice_ids (int [batch]), utterance b is spoken by voice voice_ids[b] of a VoicesPlan (gvtm_stream_create_voices)."""

    def __init__(self, plan, batch, voice_ids=None):
        self._plan = plan  # keeps the plan alive
        self._lib = plan._lib
        self._h = ctypes.c_void_p()
        self.batch = int(batch)
        self._listener = None
        if voice_ids is None:
            plan._check(self._lib.gvtm_stream_create(plan._h, self.batch, ctypes.byref(self._h)))
        else:
            ids = self._ids(voice_ids)
            plan._check(self._lib.gvtm_stream_create_voices(plan._h, _ptr(ids), self.batch, ctypes.byref(self._h)))

    def _ids(self, voice_ids):
        ids = np.ascontiguousarray(voice_ids, dtype=np.int32)
        if ids.ndim != 1 or ids.shape[0] != self.batch:
            raise ValueError("voice_ids must hold one voice id per utterance (%d), got shape %s" % (self.batch, ids.shape))
        return ids

    def close(self):
        if self._h:
            self._lib.gvtm_stream_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, voice_ids=None):
        """Every utterance back to its fresh state; with voice_ids, the utterances then take those voices."""
        if voice_ids is None:
            self._plan._check(self._lib.gvtm_stream_reset(self._h))
        else:
            self._plan._check(self._lib.gvtm_stream_reset_voices(self._h, _ptr(self._ids(voice_ids))))

    def capacity(self, max_new_frames):
        return int(self._lib.gvtm_stream_capacity(self._h, int(max_new_frames)))

    def push(self, params, frame_counts=None, audio=True):
        """params float32 [batch][F][16] -> list of float32 arrays, the new samples of each utterance.  audio=False (a listening
        stream only): no sample leaves the device -> int64 [batch], the samples synthesized."""
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.ndim == 3 and params.shape[0] == self.batch and params.shape[2] == N_PARAM
        frames = params.shape[1]
        stride = self.capacity(frames)
        out = np.zeros((self.batch, stride), dtype=np.float32) if audio else None
        counts = np.zeros(self.batch, dtype=np.int64)
        fc = None
        if frame_counts is not None:
            fc = np.ascontiguousarray(frame_counts, dtype=np.int32)
        self._plan._check(self._lib.gvtm_stream_push(self._h, _ptr(params), _ptr(fc), frames, _ptr(out), stride, _ptr(counts)))
        return self._samples(out, counts)

    def push_events(self, utterances, stride=None, audio=True):
        """gvtm_stream_push_events.  utterances[b]: the event tables (float64 [E][38] rows, events_from_table) of the chunks
        utterance b receives in this push, possibly none -> (list of float32 arrays, the new samples of each utterance;
        int32 [batch], the frames generated per utterance).  stride: the audio row length, by default capacity() of the
        largest frame total of the push.  audio=False (a listening stream only): int64 [batch] in the samples' place."""
        assert len(utterances) == self.batch
        events, chunk_offsets, utt_chunks = Plan.pack_event_lists(utterances)
        if stride is None:
            # the frames of a list follow from its times and the control period alone, the plan's 1000 / control rate
            counter = TrackConfig()
            counter.control_period_ms = int(round(1000.0 / self._plan.info.control_rate))
            new = [tracks_chunks_frame_count(counter, events[chunk_offsets[utt_chunks[b]]: chunk_offsets[utt_chunks[b + 1]]],
                                             chunk_offsets[utt_chunks[b]: utt_chunks[b + 1] + 1] - chunk_offsets[utt_chunks[b]])
                   for b in range(self.batch)]
            stride = self.capacity(max(new))
        out = np.zeros((self.batch, max(int(stride), 1)), dtype=np.float32) if audio else None
        counts = np.zeros(self.batch, dtype=np.int64)
        frames = np.zeros(self.batch, dtype=np.int32)
        self._plan._check(self._lib.gvtm_stream_push_events(self._h, _ptr(events), _ptr(chunk_offsets), _ptr(utt_chunks), _ptr(out),
                                                            int(stride), _ptr(counts), _ptr(frames)))
        return self._samples(out, counts), frames

    def targets_capacity(self, max_new_steps):
        """gvtm_stream_targets_capacity: the row length for a push_targets or finish that adds up to max_new_steps steps."""
        return _count(self._lib, int(self._lib.gvtm_stream_targets_capacity(self._h, int(max_new_steps))))

    def targets_points(self):
        """gvtm_stream_targets_points -> int64 [batch]: the points the stream holds for each utterance."""
        held = np.zeros(self.batch, dtype=np.int64)
        self._plan._check(self._lib.gvtm_stream_targets_points(self._h, _ptr(held)))
        return held

    def targets_sums(self):
        """gvtm_debug_stream_targets_sums (a stream of a diagnostics model 5 plan) -> float64 [batch][16]: the targets filters'
        sums as every utterance's block of the device state holds them."""
        if not self._plan.diagnostics:
            raise ValueError("targets_sums reads the state through a hook of the diagnostics library: make the plan with diagnostics=True")
        sums = np.zeros((self.batch, N_PARAM), dtype=np.float64)
        self._plan._check(self._lib.gvtm_debug_stream_targets_sums(self._h, _ptr(sums)))
        return sums

    def push_targets(self, utterances, step_counts, max_steps=None, audio=True):
        """gvtm_stream_push_targets.  utterances[b]: utterance b's 16 lists of (steps, values), the steps counted from the
        first step this push adds; step_counts: the steps each utterance advances by (an int: all of them by that many) ->
        list of float32 arrays, the new samples of each utterance.  A refused push raises GvtmError, whose `statuses` are
        the utterances' (int32 [batch]).  audio=False (a listening stream only): no sample leaves the device -> int64
        [batch], the samples synthesized."""
        return self._push_targets(self._lib.gvtm_stream_push_targets, utterances, step_counts, max_steps, audio)

    def push_targets_model5(self, utterances, step_counts, max_steps=None, audio=True):
        """push_targets for a stream of a one-voice model 5 plan of either class (gvtm_stream_push_targets_model5): the samples
        are the interactive window's model's, in pieces of gvtm_synthesize_targets_model5_device's."""
        return self._push_targets(self._lib.gvtm_stream_push_targets_model5, utterances, step_counts, max_steps, audio)

    def push_targets_voices(self, utterances, step_counts, max_steps=None, audio=True):
        """push_targets under the stream's own voices (gvtm_stream_push_targets_voices; a VoicesPlan of the models 0 to 4, or
        a one-voice plan): utterance b walks its lists through its voice's filter, in pieces of
        gvtm_synthesize_targets_voices_device's samples."""
        return self._push_targets(self._lib.gvtm_stream_push_targets_voices, utterances, step_counts, max_steps, audio)

    def push_targets_model5_voices(self, utterances, step_counts, max_steps=None, audio=True):
        """push_targets_model5 under the stream's own voices (gvtm_stream_push_targets_model5_voices; a model 5 plan of several
        voices of either class, or a one-voice one): in pieces of gvtm_synthesize_targets_model5_voices_device's samples."""
        return self._push_targets(self._lib.gvtm_stream_push_targets_model5_voices, utterances, step_counts, max_steps, audio)

    def _push_targets(self, entry, utterances, step_counts, max_steps, audio=True):
        assert len(utterances) == self.batch and all(len(u) == N_PARAM for u in utterances)
        counts_in = None if isinstance(step_counts, int) else np.ascontiguousarray(step_counts, dtype=np.int32)
        assert counts_in is None or counts_in.shape == (self.batch,)
        if max_steps is None:
            max_steps = step_counts if counts_in is None else max(int(counts_in.max()), 0)
        offsets, steps, values = pack_targets([l for u in utterances for l in u])
        stride = self.targets_capacity(max_steps)
        out = np.zeros((self.batch, stride), dtype=np.float32) if audio else None
        counts = np.zeros(self.batch, dtype=np.int64)
        statuses = np.full(self.batch, -1, dtype=np.int32)
        rc = entry(self._h, _ptr(offsets), _ptr(steps), _ptr(values), _ptr(counts_in), int(max_steps), _ptr(out), stride, _ptr(counts), _ptr(statuses))
        if rc != 0:
            error = GvtmError(rc, self._lib.gvtm_last_error().decode() or self._lib.gvtm_status_string(rc).decode())
            error.statuses = statuses
            raise error
        return self._samples(out, counts)

    def get_drift(self):
        """-> float64 [batch][5]: the drift generators' states (seed, x1, x2, y1, y2), one per utterance."""
        states = np.zeros((self.batch, 5), dtype=np.float64)
        self._plan._check(self._lib.gvtm_stream_get_drift(self._h, _ptr(states)))
        return states

    def set_drift(self, states=None):
        """states float64 [batch][5], or None: fresh generators (the one call that reseeds them)."""
        if states is not None:
            states = np.ascontiguousarray(states, dtype=np.float64)
            assert states.shape == (self.batch, 5)
        self._plan._check(self._lib.gvtm_stream_set_drift(self._h, _ptr(states)))

    def finish(self, audio=True):
        """-> (list of float32 arrays, maxabs float32 [batch]); audio=False (a listening stream only): int64 [batch], the
        samples synthesized, in the arrays' place."""
        stride = self.capacity(0)
        out = np.zeros((self.batch, stride), dtype=np.float32) if audio else None
        counts = np.zeros(self.batch, dtype=np.int64)
        maxabs = np.zeros(self.batch, dtype=np.float32)
        self._plan._check(self._lib.gvtm_stream_finish(self._h, _ptr(out), stride, _ptr(counts), _ptr(maxabs)))
        return self._samples(out, counts), maxabs

    def _samples(self, out, counts):
        """What a push or finish returns for its samples: each utterance's new ones, or without audio their counts."""
        if out is None:
            return counts
        return [out[b, : counts[b]].copy() for b in range(self.batch)]

    def listen(self, analysis, max_buffers, spectra=True, signal=False):
        """gvtm_stream_listen: from here on (a fresh stream) every utterance keeps the interactive window's analysis ring on the
        device, and each push queues the views of the rings it completes, max_buffers per utterance between two takes."""
        views = (LISTEN_SPECTRA if spectra else 0) | (LISTEN_SIGNAL if signal else 0)
        self._plan._check(self._lib.gvtm_stream_listen(self._h, analysis._h, int(max_buffers), views))
        self._listener = (analysis, int(max_buffers), bool(spectra), bool(signal))  # (keeps the analysis object alive)

    def unlisten(self):
        self._plan._check(self._lib.gvtm_stream_unlisten(self._h))
        self._listener = None

    def listen_state(self):
        """-> (int64 [batch], the samples in each ring; int32 [batch], the buffers queued)"""
        fill, queued = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        self._plan._check(self._lib.gvtm_stream_listen_state(self._h, _ptr(fill), _ptr(queued)))
        return fill, queued

    def take_spectra(self, fill=np.nan, copy=True):
        """gvtm_stream_take_spectra -> (spectra float32 [batch][max_buffers][n_bins] or None, signal float32
        [batch][max_buffers][W] or None, int32 [batch] the buffers taken); rows behind an utterance's count keep `fill`.
        copy=False: the queues are only emptied -> (None, None, counts)."""
        analysis, max_buffers, spectra, signal = self._listener
        spec = np.full((self.batch, max_buffers, analysis.n_bins), fill, dtype=np.float32) if spectra and copy else None
        sig = np.full((self.batch, max_buffers, analysis.window_size), fill, dtype=np.float32) if signal and copy else None
        taken = np.zeros(self.batch, dtype=np.int32)
        self._plan._check(self._lib.gvtm_stream_take_spectra(self._h, _ptr(spec), _ptr(sig), _ptr(taken)))
        return spec, sig, taken

    def peek_spectra_device(self):
        """gvtm_stream_peek_spectra_device -> (d_spectra, d_signal, d_queued): device addresses (int; None for a view not
        kept) of the queues in take_spectra's layout and of the int32 [batch] queued counts, valid until the next call on
        the stream."""
        pointers = [ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()]
        self._plan._check(self._lib.gvtm_stream_peek_spectra_device(self._h, *[ctypes.byref(p) for p in pointers]))
        return tuple(p.value for p in pointers)
