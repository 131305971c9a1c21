"""The case table of tests/test_voice_keys_cpu.py (CPU), tests/test_gpu_voice_keys.py (GPU) and
tests/golden/make_voice_keys_golden.py: the voice-configuration keys that every other test leaves at the one value of
tests/golden/voice_male.txt (voice5_male.txt for reference model 5), moved.

With them move the constants that csrc/vtm_design.cpp derives from them, in double and in float: the internal rate and
the steps per frame (temperature), damping (loss_factor), the radiation and nasal-aperture filters (mouth_coefficient,
nose_coefficient), the throat low-pass and its gain, the crossmix factor (mix_offset), the wavetable's divisions
(glottal_pulse_tp), the fixed nasal junctions and the velum's aperture, and the scale of every oral radius.

    acoustics   temperature 25 gives 79 / 158 / 238 steps per 250 Hz frame (SectionDelay 1 / 2 / 3 and the wide tube), and 79
                is prime against every chunk length
    throat_mix  the throat filter, its gain and the crossmix factor away from their shipped values
    pulse       512 * tp / 100 = 179.5: a tie of rint() whose side depends on how tp / 100 rounds in the design's type
    nose        two equal nasal radii: a junction coefficient of exactly 0
    radii       every oral radius coefficient the goldens leave at 1
    limits      mix_offset 60 is amplitude60dB()'s exact-1 branch, throat_volume 0 a gain of 0, loss_factor 0 a damping of
                1; a mouth_coefficient above Nyquist at SectionDelay 1 makes the aperture coefficient negative
    hot         temperature 40 with a shorter tract: 87 / 174 / 262 steps per frame

Needs the oracle binding and the constants of gama_tts_amd.capi only, no built library."""
import collections
import itertools

import numpy as np

from gama_tts_amd import capi
import tracks

# ---- models 0 to 4: overrides on voice_male.txt -----------------------------------------------------------------------------
SETS = collections.OrderedDict([
    ("acoustics", dict(temperature=25.0, loss_factor=0.5, mouth_coefficient=4000.0, nose_coefficient=6000.0)),
    ("throat_mix", dict(throat_cutoff=1200.0, throat_volume=9.0, mix_offset=54.0, breathiness=2.5)),
    ("pulse", dict(glottal_pulse_tp=35.05859375, glottal_pulse_tn_min=20.0, glottal_pulse_tn_max=30.0)),
    ("nose", dict(aperture_radius=2.5, nasal_radius_1=1.1, nasal_radius_2=1.5, nasal_radius_3=1.5, nasal_radius_4=1.0,
                  nasal_radius_5=0.9)),
    ("radii", dict(radius_1_coef=0.8, radius_2_coef=1.1, radius_4_coef=0.9, radius_5_coef=1.2, radius_6_coef=0.95,
                   radius_7_coef=1.05, radius_8_coef=0.85)),
    ("limits", dict(mix_offset=60.0, throat_volume=0.0, loss_factor=0.0, mouth_coefficient=12000.0, nose_coefficient=9000.0,
                    throat_cutoff=4000.0, breathiness=0.0)),
    ("hot", dict(temperature=40.0, vocal_tract_length=16.3)),
])
# steps per 250 Hz frame at SectionDelay 1 / 2 / 3 (the wide tube has SectionDelay 3's) where a set moves them
STEPS = {"acoustics": (79, 158, 238), "hot": (87, 174, 262)}
MALE_STEPS = (80, 160, 240)

# the keys of gvtm_config that no test outside this table moves
KEYS = ("temperature", "loss_factor", "mouth_coefficient", "nose_coefficient", "throat_cutoff", "throat_volume", "mix_offset",
        "glottal_pulse_tp", "aperture_radius") + tuple("nasal_radius_%d" % i for i in range(1, 6)) + tuple(
            "radius_%d_coef" % i for i in (1, 2, 4, 5, 6, 7, 8))

# ---- reference model 5: overrides on voice5_male.txt ------------------------------------------------------------------------
SETS5 = collections.OrderedDict([
    ("m5_acoustics", dict(temperature=25.0, loss_factor=0.5, mix_offset=54.0, glottal_pulse_tp=35.0, min_glottal_loss=0.5,
                          max_glottal_loss=4.0, glottal_lowpass_cutoff=6000.0, glottal_noise_cutoff=3000.0,
                          frication_noise_cutoff=5000.0, frication_factor=0.7)),
    ("m5_shape", dict(nasal_radius_2=1.5, nasal_radius_3=2.2, nasal_radius_4=1.0, nasal_radius_5=0.9, nasal_radius_6=1.2,
                      nasal_radius_7=0.8, **SETS["radii"])),
])
# the keys of gvtm5_config that no test outside this table moves (nasal_radius_2 and _3 are variant keys of 5_male, but all
# five variants have one value), the three that one vector moves all together, and glottal_lowpass_cutoff, which the male
# voice alone has at 4000 Hz and the other four at 3000 Hz
KEYS5 = ("temperature", "mix_offset", "glottal_pulse_tp") + tuple("nasal_radius_%d" % i for i in range(2, 8)) + tuple(
    "radius_%d_coef" % i for i in (1, 2, 4, 5, 6, 7, 8)) + ("glottal_noise_cutoff", "frication_noise_cutoff", "frication_factor",
                                                           "glottal_lowpass_cutoff", "loss_factor", "min_glottal_loss", "max_glottal_loss")
RATE5, CRATE = 48000.0, 250.0
MODELS5 = (("5", 0), ("5f", 1))  # (reference model string, float_model)

# what the completeness test leaves out of a configuration's fields: not voice keys, and the switches the goldens move
STRUCTURAL = ("output_rate", "section_delay", "precision", "tube_layout", "reserved_")
FLAGS = ("waveform", "noise_modulation", "bypass", "constant_radius_mouth_impedance")


def owner(key, sets=None):
    """The first set of the table that moves `key`."""
    return next(name for name, ov in (SETS if sets is None else sets).items() if key in ov)


def field_keys(config_type):
    """The fields of capi.Config / capi.Config5 by the names of the voice files' keys (arrays one key per element)."""
    first_nasal = 2 if config_type is capi.Config5 else 1
    out = []
    for name, ctype in config_type._fields_:
        if name == "nasal_radius":
            out += ["nasal_radius_%d" % (first_nasal + i) for i in range(ctype._length_)]
        elif name == "radius_coef":
            out += ["radius_%d_coef" % (1 + i) for i in range(ctype._length_)]
        else:
            out.append(name)
    return out


# ---- the one track -----------------------------------------------------------------------------------------------------------
FRAMES = 24
CUTS = (0, 1, 2, 13, 24)
# six utterances: in a four-row workgroup rows of different length and an empty row, the second workgroup half empty
BATCH_FRAMES = (24, 0, 13, 1, 2, 24)
STREAM_PIECES = (1, 6, 2, 9, 6)
COUNT_FRAMES = (0, 1, 2, 13, 24, 500)


def track():
    return tracks.random_track(FRAMES, 5, True)


def batch(frames=BATCH_FRAMES):
    """Cuts of the track as a padded batch -> (params [B][FRAMES][16], zero beyond each cut; frame counts)."""
    tr = track()
    params = np.zeros((len(frames), FRAMES, 16), np.float32)
    for b, f in enumerate(frames):
        params[b, :f] = tr[:f]
    return params, np.array(frames, dtype=np.int32)


# ---- cells -------------------------------------------------------------------------------------------------------------------
Cell = collections.namedtuple("Cell", "name precision delay layout rate model float_model")
CELLS = (
    Cell("f64-d1-44k", capi.PRECISION_F64, 1, 0, 44100.0, "0", 0),
    Cell("mixed-d1-44k", capi.PRECISION_MIXED, 1, 0, 44100.0, "0", 0),
    Cell("f32-d1-44k", capi.PRECISION_F32, 1, 0, 44100.0, "1", 1),
    Cell("f64-d2-44k", capi.PRECISION_F64, 2, 0, 44100.0, "2:2", 0),
    Cell("f32-d3-44k", capi.PRECISION_F32, 3, 0, 44100.0, "2f:3", 1),   # down-sampling
    Cell("f64-wide-44k", capi.PRECISION_F64, 1, 1, 44100.0, "4", 0),    # down-sampling
    Cell("f32-wide-22k", capi.PRECISION_F32, 1, 1, 22050.0, "4f", 1),   # down-sampling
)
CELL_IDS = [c.name for c in CELLS]
STREAM_CELLS = tuple(c for c in CELLS if c.name in ("f32-d1-44k", "f64-d2-44k"))


def steps_index(cell):
    """Index into STEPS / MALE_STEPS: the wide tube runs at SectionDelay 3's internal rate."""
    return 2 if cell.layout else cell.delay - 1


def shape_matrix_id(cell, rows):
    """The id of shape_matrix_cases' cell with this one's precision, tube and converter direction (every set keeps the
    male voice's direction: 20 to 22 kHz, 40 to 44 kHz and 60 to 65 kHz internal)."""
    pname = {capi.PRECISION_F64: "f64", capi.PRECISION_MIXED: "mixed", capi.PRECISION_F32: "f32"}[cell.precision]
    internal = (20034, 40068, 60102)[steps_index(cell)]
    return "%s-%s-%s-rows%d" % (pname, "wide" if cell.layout else "d%d" % cell.delay, "up" if cell.rate >= internal else "down", rows)


def fixture_key(set_name, model):
    return "%s__m%s" % (set_name, model.replace(":", "d"))


def reference_runs():
    """[(fixture key, overrides, voice file is model 5's, reference model string, output rate)]: every set under the model
    string and rate of every cell (two cells share model "0"), both model 5 sets in both classes."""
    runs, seen = [], set()
    for name, ov in SETS.items():
        for c in CELLS:
            if (name, c.model) not in seen:
                seen.add((name, c.model))
                runs.append((fixture_key(name, c.model), ov, False, c.model, c.rate))
    for name, ov in SETS5.items():
        for model, _ in MODELS5:
            runs.append((fixture_key(name, model), ov, True, model, RATE5))
    return runs


# ---- plans of several voices -------------------------------------------------------------------------------------------------
VOICE_NAMES = ("male",) + tuple(SETS)
# voice v of the plan is VOICE_NAMES[ORDERS[order][v]]: the male voice first, and last
ORDERS = collections.OrderedDict([("male_first", tuple(range(len(VOICE_NAMES)))),
                                  ("male_last", tuple(range(1, len(VOICE_NAMES))) + (0,))])
VOICE_NAMES5 = ("male",) + tuple(SETS5)


def overrides_of(name):
    return {} if name == "male" else (SETS[name] if name in SETS else SETS5[name])


def voice_lists():
    """The override dictionaries of the plans of several voices, per order."""
    return {order: [overrides_of(VOICE_NAMES[i]) for i in idx] for order, idx in ORDERS.items()}


def separating_pair(key, names=VOICE_NAMES):
    """Two voices of a list whose values of `key` differ, or None."""
    for a, b in itertools.combinations(names, 2):
        if overrides_of(a).get(key) != overrides_of(b).get(key):
            return a, b
    return None


def voices_batch(n_voices, seed=17):
    """Three utterances per voice, ids interleaved by a seeded permutation; voice v's are the whole track, 13 frames and
    one of 0 / 1 / 2 frames -> (params, ids, frame counts)."""
    ids = np.repeat(np.arange(n_voices, dtype=np.int32), 3)
    frames = np.concatenate([[FRAMES, 13, (0, 1, 2)[v % 3]] for v in range(n_voices)])
    perm = np.random.default_rng(seed).permutation(ids.size)
    params, frames = batch(tuple(int(f) for f in frames[perm]))
    return params, ids[perm], frames
