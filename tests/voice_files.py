"""The voice files of the tests, by name: the five GamaTTS variants of data/voice/english/0_male (tests/golden/voice_*.txt:
vocal tract 17.5 / 15 / 12.5 / 10 / 7.5 cm) and of 5_male, their reference model 5 counterparts (voice5_*.txt), and a voice
directory made of one.  Needs the oracle binding only, not the product: the fixture lists and the scripts under
tests/golden/ import it."""
import os

import oracle

# voice id v of the tests' mixed plans is VOICES[v]
VOICES = ["male", "female", "large_child", "small_child", "baby"]

# the keys that data/voice/english/0_male and 5_male keep in variant/<name>.txt, not in vtm.txt
VARIANT_KEYS = ("vocal_tract_length", "glottal_pulse_tp", "glottal_pulse_tn_min", "glottal_pulse_tn_max",
                "reference_glottal_pitch", "breathiness", "aperture_radius", "intonation_factor")
VARIANT_KEYS5 = ("vocal_tract_length", "glottal_pulse_tp", "glottal_pulse_tn_min", "glottal_pulse_tn_max",
                 "reference_glottal_pitch", "breathiness", "intonation_factor", "nasal_radius_2", "nasal_radius_3")


def voice_path(name, model5=False):
    return os.path.join(oracle.GOLDEN_DIR, "voice%s_%s.txt" % ("5" if model5 else "", name))


def write_voice_dir(root, keys, variant_keys):
    """The voice directory gama_vtm_batch reads, in GamaTTS's layout, with one variant, male: `keys` split into vtm.txt and
    variant/male.txt."""
    os.makedirs(os.path.join(root, "variant"))
    with open(os.path.join(root, "_index.txt"), "w") as f:
        f.write("variant_dir = variant/\nvtm_control_model_file = vtm_control_model.txt\nvtm_file = vtm.txt\n")
    with open(os.path.join(root, "vtm.txt"), "w") as f:
        f.write("# test voice\n")
        for k, v in keys.items():
            if k not in variant_keys:
                f.write("%s = %s\n" % (k, v))
    with open(os.path.join(root, "variant", "male.txt"), "w") as f:
        for k in variant_keys:
            f.write("%s = %s\n" % (k, keys[k]))
    with open(os.path.join(root, "vtm_control_model.txt"), "w") as f:
        f.write("control_period = 4\nvariant_name = male\n")
