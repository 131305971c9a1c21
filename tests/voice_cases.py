"""Product configurations and plans of the voices of voice_files.py: the five 0_male variants and their reference model 5
counterparts (fixture list and oracle configuration of the latter: model5_cases.py); the plan of the male voice with
overrides that the parity tests start from, the model 5 plan of any voice in either class; utterances to a padded batch
and through a stream in pieces; and a ragged batch that mixes the voices."""
import ctypes

import numpy as np

import gama_tts_amd as g
from gama_tts_amd import capi
import oracle
import tracks
from voice_files import VOICES, voice_path


def male_plan(overrides=None, rate=44100.0, delay=1, crate=250.0, precision=capi.PRECISION_F64, layout=0, rows=0, diagnostics=None,
              device=0):
    """A plan of the male voice with `overrides` on its file.  rows != 0: a plan of the diagnostics library (same kernels)
    with that many utterances per workgroup forced; diagnostics=True asks for that library with nothing forced.
    device=capi.DEVICE_NONE: a design-only plan."""
    d = g.read_config_file(oracle.VOICE_MALE)
    d.update({k: str(v) for k, v in (overrides or {}).items()})
    return g.Plan(g.config_from_dict(d, rate, delay, precision, layout), crate, device,
                  diagnostics=bool(rows) if diagnostics is None else diagnostics, rows=rows)


def model5_plan(voice="male", overrides=None, rate=48000.0, crate=250.0, rows=0, float_class=False, device=0, diagnostics=None):
    """The same for reference model 5 and one of its five voices: VocalTractModel5<double,1> (rows 1: one tube wavefront,
    chunk 60; 2: two, chunk 24) or, float_class=True, VocalTractModel5<float,1> (rows 1: chunk 60; 2: chunk 56).
    device=capi.DEVICE_NONE: a design-only plan."""
    d = g.read_config_file(voice_path(voice, True))
    d.update({k: str(v) for k, v in (overrides or {}).items()})
    cfg = g.config5_from_dict(d, rate, capi.PRECISION_F32 if float_class else capi.PRECISION_F64)
    return g.Plan(cfg, crate, device, diagnostics=bool(rows) if diagnostics is None else diagnostics, rows=rows,
                  float_model5=float_class)


def male5_plan(overrides=None, rate=48000.0, crate=250.0, rows=0):
    return model5_plan("male", overrides, rate, crate, rows)


def padded(utterances):
    """Utterances of different lengths -> (params [B][max frames][16], frame counts)."""
    frames = np.array([u.shape[0] for u in utterances], dtype=np.int32)
    params = np.zeros((len(utterances), max(1, int(frames.max())), 16), np.float32)
    for b, u in enumerate(utterances):
        params[b, : u.shape[0]] = u
    return params, frames


def push_in_pieces(plan, batch, total, pieces, voice_ids=None):
    """The utterances of `batch` (total[b] frames each) pushed into a stream in pieces of at most pieces[i] frames, then
    finished -> (samples per utterance, maxabs).  voice_ids: utterance b's voice, on a plan of several voices."""
    st = g.Stream(plan, len(total), voice_ids=voice_ids)
    outs = [[] for _ in total]
    done = np.zeros(len(total), dtype=np.int32)
    lockstep = len(set(int(t) for t in total)) == 1
    for n in pieces:
        fc = np.minimum(n, total - done).astype(np.int32)
        buf = np.zeros((len(total), n, 16), np.float32)
        for b in range(len(total)):
            buf[b, : fc[b]] = batch[b, done[b]: done[b] + fc[b]]
        res = st.push(buf, None if lockstep else fc)
        for b in range(len(total)):
            outs[b].append(res[b])
        done += fc
    assert (done == total).all()
    tails, maxabs = st.finish()
    return [np.concatenate(outs[b] + [tails[b]]) for b in range(len(total))], maxabs


def configs(rate=44100.0, delay=1, precision=capi.PRECISION_F64, layout=0, names=VOICES):
    return [g.config_from_dict(g.read_config_file(voice_path(n)), rate, delay, precision, layout) for n in names]


def configs5(rate=48000.0, names=VOICES):
    return [g.config5_from_dict(g.read_config_file(voice_path(n, True)), rate) for n in names]


def oracle_config(name, rate, delay, layout, precision):
    return oracle.config_from_dict(oracle.read_config_file(voice_path(name)), rate, delay, layout,
                                   1 if precision == capi.PRECISION_F32 else 0)


def create(cfgs, n=None, control_rate=250.0):
    """gvtm_plan_create_voices or gvtm_plan_create_model5_voices (by the configurations' type) for a design-only plan ->
    (status, handle); a plan that was made is destroyed again."""
    lib = g.load_library()
    h = ctypes.c_void_p()
    model5 = bool(cfgs) and isinstance(cfgs[0], capi.Config5)
    arr = ((capi.Config5 if model5 else capi.Config) * len(cfgs))(*cfgs) if cfgs else None
    make = lib.gvtm_plan_create_model5_voices if model5 else lib.gvtm_plan_create_voices
    rc = make(arr, len(cfgs) if n is None else n, control_rate, capi.DEVICE_NONE, ctypes.byref(h))
    if rc == 0:
        lib.gvtm_plan_destroy(h)
    return rc, h


def track_configs(names=VOICES, model5=False):
    """A voice's track configuration as Controller.cpp:70-81 sets its EventList up: 0_male/vtm_control_model.txt (control
    period 4, pitch offset -4, initial pitch -20, drift deviation 4 at 250 Hz with a 4 Hz low-pass, every intonation flag on)
    and mean pitch = pitch offset + the reference_glottal_pitch of the voice's variant file."""
    out = []
    for n in names:
        c = g.TrackConfig()
        c.control_period_ms = 4
        c.macro_intonation = c.micro_intonation = c.intonation_drift = c.smooth_intonation = 1
        c.initial_pitch = -20.0
        c.mean_pitch = -4.0 + float(g.read_config_file(voice_path(n, model5))["reference_glottal_pitch"])
        c.drift_deviation, c.drift_sample_rate, c.drift_lowpass_cutoff = 4.0, 250.0, 4.0
        out.append(c)
    return out


def mixed_batch(batch, max_frames, n_voices, seed):
    """Interleaved, ragged ids; 0-, 1- and 2-frame utterances of every voice."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n_voices, size=batch).astype(np.int32)
    ids[: 3 * n_voices] = np.repeat(np.arange(n_voices, dtype=np.int32), 3)
    frames = rng.integers(3, max_frames + 1, size=batch).astype(np.int32)
    frames[: 3 * n_voices] = np.tile([0, 1, 2], n_voices)
    perm = rng.permutation(batch)
    params = tracks.random_tracks(batch, max_frames, seed0=seed, consonant_heavy=True)
    return params, ids[perm], frames[perm]


# (precision, SectionDelay, output rate, tube layout) of the mixed-voice launches and streams
CASES = [(capi.PRECISION_F32, 1, 44100.0, 0), (capi.PRECISION_F32, 2, 44100.0, 0),
         (capi.PRECISION_MIXED, 1, 44100.0, 0), (capi.PRECISION_MIXED, 2, 44100.0, 0),
         (capi.PRECISION_F64, 1, 44100.0, 0), (capi.PRECISION_F64, 2, 44100.0, 0),
         (capi.PRECISION_F64, 1, 22050.0, 1)]
CASE_IDS = ["f32-d1", "f32-d2", "mixed-d1", "mixed-d2", "f64-d1", "f64-d2", "f64-layout1-22k"]
