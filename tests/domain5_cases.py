"""Reference model 5 on parameter frames OUTSIDE the editor's ranges: the table of tests/domain_cases.py for
VocalTractModel5, its track builder, its float predicate and the loader of the vectors the REAL reference made for it
(tests/golden/make_domain5_golden.py -> tests/golden/vtm5_domain_golden.npz).  Shared by tests/test_domain5_cpu.py (the
oracle in both classes) and tests/test_gpu_domain5.py (the four code objects of csrc/vtm_kernel_m5.inc).

The contract is "what the reference computes".  VocalTractModel5::vocalTract (vtm/VocalTractModel5.h:716-726) adds the
frication to oropharynx_[S6 + (int)(22 * fricPos / 7)], an array of 30 sections: the index stays inside it for every
position in about (-1.909, 7.954), which covers S1 (positions down to -1.9) and S29 / S30 (7.32 to 7.95).  In all of that
range, and for every other parameter at any finite value, the reference is plain defined C++: volumes above 60 dB and
below 0, radii at and below 0 (std::max(..., 0.01)), velum at and below 0, centre frequencies and bandwidths beyond the
Nyquist rate or negative, far pitches, the Rosenberg t2 of an amplitude above 1 when tn_min != tn_max, the radiation
impedance of a clamped r8.

Classes: "5" = VocalTractModel5<double,1>, "5f" = VocalTractModel5<float,1>, at 44 100 Hz with a 250 Hz control rate.
Voices: 5_male gets every case; female and baby the SUBSET (the edge frication positions on the frication-only base, all
radii 0, pitch 70, fricCF 9e5).  VARIANTS are 5_male with one override each, and get the cases that move the override's
own path.  A bandwidth case is a FACTOR of the MALE internal rate (MALE_FS, the lowest of the five voices), so that it
never exceeds half of any voice's rate.

Two bases: B = domain_cases.base_frame(); F = the same with glotVol 0, aspVol 0, fricVol 60, frication only: on it a
misplaced frication share is half the signal, not a per cent of it.

Track forms: "plateau" = base, base, X, X, X, X, base, base (X the base with the case's overrides), so that the per-step
interpolation passes through the whole range in both directions; "const" = eight frames X; "ramp" = eight frames from the
base to X in equal steps.

reference=False marks the PRODUCT-RULE cases: positions whose section lies outside S1..S30.  The reference indexes its
array out of bounds there, there is nothing to be equal to, and no vector: the product's rule (oracle/vtm_oracle_body.inc,
csrc/vtm_kernel_m5.inc) is that nothing is injected.  Their const tracks must therefore equal the same frames with
fricVol 0 and fricPos 3.5 (PRODUCT_NEUTRAL), numerically.

Left out on purpose:
  * NaN / Inf parameters: the reference's (int) cast of them is undefined, and they poison every later sample;
  * bandwidths above half the internal rate: an unstable band-pass, the reference's output is inf / NaN.
"""
import functools
import hashlib
import json
import os

import numpy as np

import domain_cases
import model5_cases
import oracle

FRAMES = 8
RATE, CRATE = 44100.0, 250.0
CLASSES = [("5", 0), ("5f", 1)]  # model string for oracle/_ref/ref_vtm, float model
VOICES = ("male", "female", "baby")
# (331.4 + 0.6 * temperature) * 30 * 100 / vocal tract length (VocalTractModel5.h:462-465): 60 411.43 Hz
MALE_FS = (331.4 + 0.6 * 35.0) * 30.0 * 100.0 / 17.5

# 5_male with an override: name -> configuration keys
VARIANTS = {
    "tn_delta": dict(glottal_pulse_tn_min=16.0, glottal_pulse_tn_max=32.0),
    "sine": dict(waveform=1),
    "const_mouth": dict(constant_radius_mouth_impedance="true"),
    "no_modulation": dict(noise_modulation=0),
}
# every configuration a vector is made in: name -> (voice file, overrides)
CONFIGS = {v: (v, {}) for v in VOICES}
CONFIGS.update({name: ("male", ov) for name, ov in VARIANTS.items()})

PRODUCT_NEUTRAL = {3: 0.0, 4: 3.5}

# S1 in the float class.  The reference adds S1's frication share to a section that already holds the tube input:
# (bottom * loss + input) + share (VocalTractModel5.h:652, :722).  The kernel's S1 lane has ONE "added" value per step, so
# it forms bottom * loss + (input + share): one float rounding away, in a recursion.  The exact form (a second addition in
# the tube loop, taken only by chunks that have such a step) was built and is bit-identical, but costs 1.2 % (double) and
# 2.3 to 3.0 % (float) of the model 5 kernels' time on frames that never come near S1 (profiles/domain5_ab.md), so the
# folded form stands and every float case whose track enters S1 is held to the mixed path's bar (parity_rules.TOL[MIXED]):
# still a guard against a wrong branch (a dropped or misplaced S1 share misses by 4 % of peak on base B, 99 % on base F).
S1_FLOAT_BAR = 1e-5
S1_REASON = "the S1 share is folded into the tube input: bottom * loss + (input + share), one float rounding from the reference"
# case name -> why the float class cannot be bit-identical on it although its arguments are inside the pinned ranges
FLOAT_BAR_REASONS = {}


def base_frame(base):
    f = domain_cases.base_frame()
    if base == "F":
        f[1], f[2], f[3] = 0.0, 0.0, 60.0
    return f


def section_index(pos, dtype):
    """5 + trunc(22 * pos / 7) as the class forms it (VocalTractModel5.h:716-722): the 0-based index into the 30
    sections, S1 = 0 ... S30 = 29."""
    pos = dtype(np.float32(pos))
    return 5 + int(np.trunc(dtype(27 - 5) * (pos / dtype(7.0))))


def D(name, configs=("male",), base="B", form="plateau", float_pinned=True, bw_factor=None, float_bar=None, reference=True,
      section=None, **overrides):
    """overrides: p<index>=value; configs: the names of CONFIGS the case is made in; section: the 0-based section index a
    frication-position case lands in; bw_factor: fricBW (6) = factor x MALE_FS; float_bar: the float class's bar for this
    case where it cannot be bit-identical (None: bit-identical inside the pinned ranges, parity_rules.TOL of the mixed path
    outside)."""
    return dict(name=name, configs=tuple(configs), base=base, form=form, float_pinned=float_pinned, bw_factor=bw_factor,
                float_bar=float_bar, reference=reference, section=section,
                overrides={int(k[1:]): float(v) for k, v in overrides.items()})


ALL3 = VOICES
CASES = []
# frication position (4), each on both bases.  The section is 5 + trunc(22 * pos / 7):
FPOS = [
    ("m1.9", -1.9, 0),     # 22 * -1.9 / 7 = -5.97 -> -5: S1, the last position inside the tube
    ("m1.85", -1.85, 0),   # -5.81 -> -5: S1
    ("m1.7", -1.7, 0),     # -5.34 -> -5: S1 (the right share goes to S2)
    ("m1.5", -1.5, 1),     # -4.71 -> -4: S2
    ("m0.5", -0.5, 4),     # -1.57 -> -1: S5
    ("m1e-3", -1e-3, 5),   # -0.003 -> 0: S6, with a NEGATIVE right share and a left share above 1
    ("7", 7.0, 27),        # 22 -> S28: no right share (the "< 27" rule, :723-725)
    ("7.2", 7.2, 27),      # 22.63 -> 22: S28, the right share is dropped
    ("7.5", 7.5, 28),      # 23.57 -> 23: S29
    ("7.8", 7.8, 29),      # 24.51 -> 24: S30
    ("7.95", 7.95, 29),    # 24.99 -> 24: S30, the last position inside the tube
]
EDGE_POSITIONS = ("m1.85", "m1.7", "7.8", "7.95")  # the subset's: S1 and S30
for _n, _pos, _sec in FPOS:
    _bar = S1_FLOAT_BAR if _sec == 0 else None
    CASES.append(D("fpos_%s_B" % _n, base="B", section=_sec, float_bar=_bar, p4=_pos))
    CASES.append(D("fpos_%s_F" % _n, ALL3 if _n in EDGE_POSITIONS else ("male",), base="F", section=_sec, float_bar=_bar, p4=_pos))
CASES += [
    # volumes (1, 2, 3) above 60 dB and below 0
    D("gvol_65", ("male", "tn_delta", "no_modulation"), p1=65.0), D("gvol_70", ("tn_delta",), p1=70.0), D("gvol_m5", p1=-5.0),
    D("avol_65", p2=65.0), D("fvol_65", p3=65.0), D("fvol_m5", p3=-5.0),
    # radii (7..14) and velum (15) at and below 0; r8 also sets the mouth's radiation impedance
    D("r1_r3_0", p7=0.0, p9=0.0), D("r2_r6_neg", p8=-0.5, p12=-1.0),
    D("radii_0", ALL3, **{"p%d" % i: 0.0 for i in range(7, 15)}), D("r8_m1", ("male", "const_mouth"), p14=-1.0),
    D("velum_m0.5", p15=-0.5), D("velum_0", p15=0.0),
    # centre frequency (5): above the Nyquist rate, negative, and a cos argument of 94 rad, beyond cosf's pinned range
    D("fcf_40k", p5=40000.0), D("fcf_m2500", p5=-2500.0), D("fcf_9e5", ALL3, float_pinned=False, p5=9.0e5),
    # bandwidth (6): tan arguments above 1.38 up to pi/2, negative (a band-pass that GROWS: the vector's peak is 1.4e12
    # against 4.2e4 elsewhere, finite), zero
    D("fbw_0.45fs", float_pinned=False, bw_factor=0.45), D("fbw_0.49fs", float_pinned=False, bw_factor=0.49),
    D("fbw_m500", p6=-500.0), D("fbw_0", p6=0.0),
    # pitch (0); the sine source's argument stays within 2 pi
    D("pitch_40", p0=40.0), D("pitch_m60", p0=-60.0), D("pitch_70", ALL3 + ("sine",), p0=70.0),
    D("pitch_90", ("male", "sine"), p0=90.0),
]
# the product's rule: sections outside S1..S30
for _n, _pos in [("m1.95", -1.95), ("m3", -3.0), ("8", 8.0), ("9", 9.0), ("40", 40.0), ("1e12", 1e12), ("m1e12", -1e12)]:
    CASES.append(D("prod_const_%s" % _n, base="F", form="const", reference=False, p4=_pos))
CASES += [D("prod_ramp_9", base="F", form="ramp", reference=False, p4=9.0),
          D("prod_ramp_m3", base="F", form="ramp", reference=False, float_bar=S1_FLOAT_BAR, p4=-3.0)]  # (crosses S1)
FLOAT_BAR_REASONS.update({c["name"]: S1_REASON for c in CASES if c["float_bar"] is not None})
BY_NAME = {c["name"]: c for c in CASES}
REFERENCE_CASES = [c for c in CASES if c["reference"]]
PRODUCT_CASES = [c for c in CASES if not c["reference"]]


def cases_of(config, reference=True):
    """The cases made in configuration `config` (a name of CONFIGS), in table order."""
    return [c for c in CASES if config in c["configs"] and c["reference"] == reference]


def track_for(case, neutral=False):
    """The case's 8 frames; neutral: with PRODUCT_NEUTRAL in place of its frication volume and position."""
    base = base_frame(case["base"])
    x = base.copy()
    for k, v in case["overrides"].items():
        x[k] = v
    if case["bw_factor"] is not None:
        x[6] = case["bw_factor"] * MALE_FS
    if case["form"] == "plateau":
        rows = [base, base, x, x, x, x, base, base]
    elif case["form"] == "const":
        rows = [x] * FRAMES
    else:
        rows = [base + (x - base) * np.float32(i / (FRAMES - 1.0)) for i in range(FRAMES)]
    t = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
    if neutral:
        for k, v in PRODUCT_NEUTRAL.items():
            t[:, k] = v
    return t


def float_pinned5(track, fs):
    """domain_cases.float_pinned for the float class of model 5 at internal rate fs: whether every argument the track
    hands to the float restatements of csrc/vtm_math.hpp stays inside the ranges on which they are pinned to libm bit for
    bit (domain_cases.PINNED) -- the band-pass design's tanf(pi fricBW / fs) and cosf(2 pi fricCF / fs)
    (BandpassFilter::update, the same statements as in the other models), powf(2, (pitch + 3) / 12) and
    powf(10, (vol - 60) / 20) (VTMUtil.h).

    Two more float arguments are formed from a frame and stay pinned for EVERY case, whatever the frame:
      * the radiation impedance's cosf(2 pi (62.3371 / r + 320.204) / fs) (PoleZeroRadiationImpedance::update): the radius
        is clamped to 0.5 cm from below, so the argument is at most 2 pi x 12 788 Hz / 60 411 Hz = 1.33 rad on the male
        voice and less on the others;
      * the sine source's sinf(2 pi t): t is wrapped at 1 after each increment of f0 / fs, so the argument stays within
        2 pi -- the range on which sinf_glibc is held to libm (tests/test_capi_model5_cpu.py) -- while one increment stays
        below a period, and within the first lap beyond for any pitch below about 97 (f0 = fs).
    """
    return domain_cases.float_pinned(track, np.float32(fs))


def oracle_config(config, float_model):
    voice, overrides = CONFIGS[config]
    return model5_cases.voice_oracle_config(voice, RATE, float_model, overrides)


def config_keys(config):
    voice, overrides = CONFIGS[config]
    return model5_cases.config_keys(dict(voice=voice, overrides=overrides))


def synthesize_many(jobs, workers=8):
    """jobs: [(configuration name, float model, track)] -> the oracle's samples, read-only, a thread per utterance (the C
    restatement keeps no global state and ctypes releases the GIL: no child process)."""
    from concurrent.futures import ThreadPoolExecutor

    oracle.lib()

    def run(job):
        out = oracle.synthesize5(oracle_config(job[0], job[1]), job[2], CRATE)[0]
        out.setflags(write=False)
        return out

    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(run, list(jobs)))


def class_key(cls):
    return "m" + cls[0]


def key(case, config, cls):
    return "%s__%s__%s" % (case["name"], config, class_key(cls))


def block_key(config, cls):
    return "%s__%s" % (config, class_key(cls))


def vector_keys():
    """[(case, configuration name, class)] of every vector of the fixture, in its order."""
    return [(case, config, cls) for cls in CLASSES for config in CONFIGS for case in cases_of(config)]


GOLDEN = os.path.join(oracle.GOLDEN_DIR, "vtm5_domain_golden.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """{key: samples, read-only} of every vector plus "manifest": {key: dict(n, offset, fs, sha256, peak)}."""
    z = np.load(GOLDEN, allow_pickle=False)
    manifest = json.loads(bytes(z["manifest_json"]).decode())
    data = {}
    blocks = {}
    for case, config, cls in vector_keys():
        bk = block_key(config, cls)
        if bk not in blocks:
            blocks[bk] = z[bk]
            blocks[bk].setflags(write=False)
        m = manifest[key(case, config, cls)]
        data[key(case, config, cls)] = blocks[bk][m["offset"]: m["offset"] + m["n"]]
    data["manifest"] = manifest
    return data


def check_against_golden(out, case, config, cls, data):
    k = key(case, config, cls)
    m = data["manifest"][k]
    ref = data[k]
    assert out.size == m["n"] == ref.size, (k, out.size, m["n"])
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"], k
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), k
