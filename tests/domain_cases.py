"""Parameter frames OUTSIDE the editor's ranges (tracks._RANGES, tracks.edge_track): one table, its track builder and the
loader of the vectors the REAL reference made for it (tests/golden/make_domain_golden.py ->
tests/golden/vtm_domain_golden.npz), shared by tests/test_domain_cpu.py (oracle) and tests/test_gpu_domain.py (kernels).

The C ABI takes any float, and the contract is "what the reference computes": negative and fractional frication
positions on both sides of setFricationTaps' loop (VocalTractModel0.h:524-552; a position in (-2, -1) leaves all eight
taps 0, because the second share is written from inside the i == integerPart branch only), volumes above 60 dB and below
0, radii and velum at and below 0, centre frequencies above the Nyquist rate and below 0, bandwidths up to half the
internal rate and below 0, pitches far outside the voice's range.

A case's track is 8 frames: base, base, X, X, X, X, base, base -- X the base frame with the case's overrides -- so the
per-step interpolation passes through the whole range in both directions.  The base frame is tracks.const_track(1)[0]
with aspVol 10 and fricVol 40: frication and aspiration are audible.  A bandwidth case is a FACTOR of the configuration's
internal rate (10 + 6 tube: 20034 Hz, at SectionDelay 2: 40068 Hz, 30 + 18 tube: 60102 Hz; the loader takes it from the manifest, a device test from
the plan's design).

Left out on purpose:
  * NaN / Inf parameters and a frication position beyond the range of int: static_cast<int> of them is undefined
    behaviour in the reference itself, there is nothing to be equal to;
  * bandwidths above half the internal rate: an unstable band-pass, the reference's output is inf / NaN.

float_pinned: every argument the track hands to the float restatements of csrc/vtm_math.hpp stays inside the ranges
on which they are pinned to libm bit for bit (PINNED below; tests/test_capi_cpu.py scans them).  Outside, the float
path takes the library fallback and last-bit differences are expected: such a case is held to the mixed bar only
(float_bar: a bar of its own where the device was measured beyond that, with the figure and the reason).  The
table's flag says "pinned at the internal rate of every class"; float_pinned(track, fs) is the predicate itself, and
tests/test_domain_cpu.py recomputes the flags from it.
"""
import hashlib
import json
import os

import numpy as np

import oracle
import tracks

FRAMES = 8

# model string for ref_vtm, SectionDelay, tube layout, float model -- the six classes every case is made in
CLASSES = [("0", 1, 0, 0), ("2:2", 2, 0, 0), ("4", 1, 1, 0), ("1", 1, 0, 1), ("2f:2", 2, 0, 1), ("4f", 1, 1, 1)]
RATE = 44100.0

# |argument| limits of the float restatements' pinned ranges: tanf on [-1.38, 1.38] and cosf on (-16, 16), every float;
# powf(10, y) and powf(2, x) on the every-float ranges of tests/test_capi_cpu.py plus its random samples of |y| < 25 and
# |x| < 90 (the same straight-line double arithmetic throughout)
PINNED = dict(tan=1.38, cos=16.0, pow10=25.0, pow2=90.0)


def base_frame():
    f = tracks.const_track(1)[0].copy()
    f[2], f[3] = 10.0, 40.0
    return f


def D(name, float_pinned=True, bw_factor=None, float_bar=None, **overrides):
    """overrides: p<index>=value; bw_factor: fricBW (6) = factor x the internal rate; float_bar: the float kernels' bar for
    this case where its arguments are outside the pinned ranges (None: parity_rules.TOL of the mixed path)."""
    return dict(name=name, float_pinned=float_pinned, bw_factor=bw_factor, float_bar=float_bar,
                overrides={int(k[1:]): float(v) for k, v in overrides.items()})


# fcf_9e5 in float, measured on an MI355X, peak-relative error against the float oracle per tube:
#   10 + 6 tube, SectionDelay 1 and 2 (cos arguments up to 282 and 141 rad): 0, every sample bit-identical;
#   30 + 18 tube (up to 94 rad), rows 1, 2 and 4 alike: 2.02e-5, 1204 of 1436 samples differing.
# The device's fallback there is (float)cos((double)y), correctly rounded, libm's cosf is within an ulp of that, and the
# band-pass the coefficient goes into has its poles at radius 0.974 (bandwidth 500 Hz at 60102 Hz): a last-bit difference in
# -(1 + a2) cos rings on in the recursion and through the four frames of the plateau.  The mixed bar (1e-5) was chosen as
# a guard against a wrong branch (those miss by 6 to 43 % of peak, tests/test_gpu_domain.py before the tap fix), not as a
# bound on that: the case's bar is four times the measured error.
FCF_9E5_FLOAT_BAR = 4 * 2.02e-5


CASES = [
    # frication position (4): both sides of every branch of the tap loop
    D("fpos_m2.5", p4=-2.5), D("fpos_m1.5", p4=-1.5), D("fpos_m1", p4=-1.0), D("fpos_m0.5", p4=-0.5),
    D("fpos_m1e-3", p4=-1e-3), D("fpos_7.5", p4=7.5), D("fpos_8.5", p4=8.5),
    # volumes (1, 2, 3) above 60 dB and below 0
    D("gvol_65", p1=65.0), D("gvol_m5", p1=-5.0), D("avol_65", p2=65.0), D("avol_m5", p2=-5.0),
    D("fvol_65", p3=65.0), D("fvol_m5", p3=-5.0),
    # radii (7..14) and velum (15) at and below 0
    D("r1_r3_0", p7=0.0, p9=0.0), D("r2_r6_neg", p8=-0.5, p12=-1.0),
    D("radii_0", **{"p%d" % i: 0.0 for i in range(7, 15)}), D("velum_m0.5", p15=-0.5), D("velum_0", p15=0.0),
    # centre frequency (5): above the Nyquist rate of both tubes, negative, and cos arguments of 18.8 and 282 on the 10 + 6
    # tube, beyond cosf's pinned range
    D("fcf_20k", p5=20000.0), D("fcf_60k", False, p5=60000.0), D("fcf_m2500", p5=-2500.0), D("fcf_9e5", False, float_bar=FCF_9E5_FLOAT_BAR, p5=9.0e5),
    # bandwidth (6): tan arguments above 1.38 up to pi/2, negative, zero
    D("fbw_0.45fs", False, bw_factor=0.45), D("fbw_0.49fs", False, bw_factor=0.49), D("fbw_0.5fs", False, bw_factor=0.5),
    D("fbw_m500", p6=-500.0), D("fbw_0", p6=0.0),
    # pitch (0)
    D("pitch_40", p0=40.0), D("pitch_m40", p0=-40.0), D("pitch_m60", p0=-60.0), D("pitch_70", p0=70.0),
]
BY_NAME = {c["name"]: c for c in CASES}


def track_for(case, fs):
    """The case's 8 frames for a configuration whose internal rate is fs."""
    base = base_frame()
    x = base.copy()
    for k, v in case["overrides"].items():
        x[k] = v
    if case["bw_factor"] is not None:
        x[6] = case["bw_factor"] * fs
    return np.ascontiguousarray(np.stack([base, base, x, x, x, x, base, base]), dtype=np.float32)


def float_pinned(track, fs):
    """Whether every argument the float conversions form from `track` lies in PINNED.  The per-step interpolation is linear
    between frames, so the arguments' extremes are the frames' own; they are formed here as the float model forms them
    (BandpassFilter.h:105-106, VTMUtil.h:48-84), and no case sits within rounding of a limit."""
    t = np.asarray(track, dtype=np.float32)
    f32 = np.float32
    T = f32(1.0) / f32(fs)
    tan_arg = f32(np.pi) * t[:, 6] * T
    cos_arg = f32(2.0) * f32(np.pi) * t[:, 5] * T
    pow2_arg = (t[:, 0] + f32(3.0)) * f32(1.0 / 12.0)
    vols = t[:, 1:4]
    pow10_arg = np.where((vols <= 0) | (vols == 60), f32(0.0), (vols - f32(60.0)) * f32(1.0 / 20.0))
    return bool(np.abs(tan_arg).max() <= PINNED["tan"] and np.abs(cos_arg).max() < PINNED["cos"]
                and np.abs(pow2_arg).max() < PINNED["pow2"] and np.abs(pow10_arg).max() < PINNED["pow10"])


def class_key(cls):
    return "m" + cls[0].replace(":", "d")


def key(case, cls):
    return "%s__%s" % (case["name"], class_key(cls))


GOLDEN = os.path.join(oracle.GOLDEN_DIR, "vtm_domain_golden.npz")


def golden():
    """{key: samples} of every case x class plus "manifest": {key: dict(n, offset, fs, sha256, peak)}."""
    z = np.load(GOLDEN, allow_pickle=False)
    manifest = json.loads(bytes(z["manifest_json"]).decode())
    data = {}
    for cls in CLASSES:
        block = z[class_key(cls)]
        for case in CASES:
            m = manifest[key(case, cls)]
            data[key(case, cls)] = block[m["offset"]: m["offset"] + m["n"]]
    data["manifest"] = manifest
    return data


def class_fs(manifest, cls):
    """The internal rate of a class (the reference's own figure, the same for every case)."""
    return manifest[key(CASES[0], cls)]["fs"]


def check_against_golden(out, case, cls, data):
    m = data["manifest"][key(case, cls)]
    ref = data[key(case, cls)]
    assert out.size == m["n"] == ref.size, (key(case, cls), out.size, m["n"])
    assert hashlib.sha256(out.tobytes()).hexdigest() == m["sha256"], key(case, cls)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), key(case, cls)
