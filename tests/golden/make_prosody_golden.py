#!/usr/bin/env python3
"""Generates tests/golden/prosody_golden.npz by running the REAL reference (build container only).

tests/golden/ref_prosody_table.cpp is compiled here against /root/reference with the whole-library flags of oracle/Makefile
(-std=c++17 -O2 -ffp-contract=off), into a temporary directory outside the repository, and fed the cases of
tests/prosody_cases.py: per case the reference's own builder calls (a text case: its text parser and PhoneticStringParser,
chunk by chunk), generateEventList() and applyIntonation().

prosody_golden.npz holds data only:
  names                      the entries, in order (a table case by its name, a text case as <name>.<chunk>)
  intonation                 float32 [8]: intonation.txt in gvtm_prosody_config's order; rhythm float64 [8]: rhythm.txt
  tone_group_param_<type>    float32 [sets][5]: the five parameter files, type 0..4
  vocoid                     uint8 [postures]: Posture::isMemberOfCategory("vocoid") of the 0_male database
  <entry>__cp, __random, __seed, __intonation_factor (float32), __global_tempo
  <entry>__postures          [n][4] id, marked, tempo BEFORE applyRhythm(), rule_tempo; __tempo_after float64 [n]
  <entry>__feet              [F][4] start, end, marked, tempo before rhythm (the closed feet); __draws float64 [F][2]: what
                             the reference drew per foot (zeros when __random is 0)
  <entry>__groups            [G][8] start_foot, end_foot, type (5: none), the parameter set intonationParameters() returned
  <entry>__rule_data         [R][8] float64; __onsets float64 [n]
  <entry>__points            float64 [P][3]: absoluteTime(), semitone(), slope() of the IntonationPoints
  <entry>__merged            float64 [E][38]: the list after applyIntonation() with macro intonation on, smooth, as
                             capi.events_from_table reads it

    python tests/golden/make_prosody_golden.py
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import prosody_cases as cases  # noqa: E402
import rules_cases  # noqa: E402
from gama_tts_amd import control_model  # noqa: E402
from make_rules_golden import FLAGS, INCLUDES, REF_SRC, REF_VOICE_DIR, text  # noqa: E402

OPS = {"foot": 1, "mark": 2, "ftempo": 3, "group": 4, "type": 5}


def build(workdir):
    """The reference's translation units (all but main.cpp) and ref_prosody_table.cpp -> workdir/ref_prosody_table"""
    import glob
    sources = [s for s in glob.glob(os.path.join(REF_SRC, "**", "*.cpp"), recursive=True) if os.path.basename(s) != "main.cpp"]
    objects, jobs = [], []
    for i, src in enumerate(sorted(sources)):
        obj = os.path.join(workdir, "%03d.o" % i)
        objects.append(obj)
        jobs.append(subprocess.Popen(["g++"] + FLAGS + INCLUDES + ["-c", "-o", obj, src]))
        if len(jobs) == 8:
            assert jobs.pop(0).wait() == 0
    for j in jobs:
        assert j.wait() == 0
    exe = os.path.join(workdir, "ref_prosody_table")
    subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(HERE, "ref_prosody_table.cpp")] + objects + ["-ldl"], check=True)
    return exe


def main():
    male = control_model.compile_model(os.path.join(REF_VOICE_DIR, "artic.xml"))
    kept = np.load(rules_cases.MODEL_0_MALE)
    assert [str(n) for n in male["posture_names"]] == [str(n) for n in kept["posture_names"]]
    ids = {str(n): i for i, n in reversed(list(enumerate(male["posture_names"])))}
    names = list(cases.CASES)
    blob = [b"GVPI", struct.pack("<i", 1), struct.pack("<i", len(names))]
    for n in names:
        c = cases.CASES[n]
        fixed = c["fixed"] or (0.0,) * 5
        blob.append(struct.pack("<iiiIi5ffd", 0 if c["text"] is None else 1, c["cp"], 0 if c["seed"] is None else 1, c["seed"] or 0,
                                0 if c["fixed"] is None else 1, *fixed, c["intonation_factor"], c["global_tempo"]))
        if c["text"] is not None:
            blob.append(text(c["text"]))
            continue
        blob.append(struct.pack("<i", len(c["ops"])))
        for op in c["ops"]:
            if op[0] == "p":
                blob.append(struct.pack("<iiidd", 0, ids[op[1]], op[2], op[3], op[4]))
            elif op[0] == "ftempo":
                blob.append(struct.pack("<id", OPS[op[0]], op[1]))
            elif op[0] == "type":
                blob.append(struct.pack("<ii", OPS[op[0]], op[1]))
            else:
                blob.append(struct.pack("<i", OPS[op[0]]))
    with tempfile.TemporaryDirectory() as td:
        exe = build(td)
        pin, pout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(pin, "wb") as f:
            f.write(b"".join(blob))
        subprocess.run([exe, REF_VOICE_DIR, pin, pout], check=True)
        data = open(pout, "rb").read()
    assert data[:4] == b"GVPO" and struct.unpack_from("<i", data, 4) == (1,)
    off = 8

    def take(dtype, count, shape=None):
        nonlocal off
        a = np.frombuffer(data, dtype=dtype, count=count, offset=off).copy()
        off += a.nbytes
        return a if shape is None else a.reshape(shape)

    out = {"intonation": take("<f4", 8), "rhythm": take("<f8", 8)}
    for t in range(5):
        n_sets = int(take("<i4", 1)[0])
        out["tone_group_param_%d" % t] = take("<f4", n_sets * 5, (n_sets, 5))
    n_postures = int(take("<i4", 1)[0])
    out["vocoid"] = take(np.uint8, n_postures)
    assert np.array_equal(out["vocoid"], male["vocoid"]), "compile_model's vocoid table is not the reference's"
    n_chunks = int(take("<i4", 1)[0])
    entries, chunk_of = [], {}
    for _ in range(n_chunks):
        ci, exception, n = (int(x) for x in take("<i4", 3))
        case = names[ci]
        c = cases.CASES[case]
        entry = case
        if c["text"] is not None:
            entry = "%s.%d" % (case, chunk_of.get(case, 0))
            chunk_of[case] = chunk_of.get(case, 0) + 1
        assert exception == 0, (entry, exception)
        postures, after = np.zeros((n, 4)), np.zeros(n)
        for i in range(n):
            pid, marked = take("<i4", 2)
            tempo, rule_tempo, after[i] = take("<f8", 3)
            postures[i] = pid, marked, tempo, rule_tempo
        n_feet = int(take("<i4", 1)[0])
        feet, draws = np.zeros((n_feet, 4)), np.zeros((n_feet, 2))
        for i in range(n_feet):
            feet[i, :3] = take("<i4", 3)
            feet[i, 3], draws[i, 0], draws[i, 1] = take("<f8", 3)
        n_groups = int(take("<i4", 1)[0])
        groups = np.zeros((n_groups, 8))
        for g in range(n_groups):
            groups[g, :3] = take("<i4", 3)
            groups[g, 3:] = take("<f4", 5)
        groups[groups[:, 2] == 6, 2] = 5  # IntonationRhythm::ToneGroup::none
        n_rules = int(take("<i4", 1)[0])
        rule_data = take("<f8", n_rules * 8, (n_rules, 8))
        onsets = take("<f8", n)
        n_points = int(take("<i4", 1)[0])
        points = take("<f8", n_points * 3, (n_points, 3))
        n_events = int(take("<i4", 1)[0])
        merged = take("<f8", n_events * 38, (n_events, 38))
        entries.append(entry)
        out[entry + "__cp"] = np.int32(c["cp"])
        out[entry + "__random"] = np.int32(0 if c["seed"] is None else 1)
        out[entry + "__seed"] = np.uint32(c["seed"] or 0)
        out[entry + "__intonation_factor"] = np.float32(c["intonation_factor"])
        out[entry + "__global_tempo"] = np.float64(c["global_tempo"])
        out[entry + "__postures"], out[entry + "__tempo_after"] = postures, after
        out[entry + "__feet"], out[entry + "__draws"], out[entry + "__groups"] = feet, draws, groups
        out[entry + "__rule_data"], out[entry + "__onsets"], out[entry + "__points"], out[entry + "__merged"] = rule_data, onsets, points, merged
        print(entry, n, "postures", n_feet, "feet", n_groups, "groups", n_rules, "rules", n_points, "points", n_events, "events")
    assert off == len(data)
    out["names"] = np.asarray(entries)
    # what the cases were written for
    assert len(out["points_64__points"]) == 64
    assert (out["delta_zero__onsets"][int(out["delta_zero__feet"][-1, 0])] == out["delta_zero__onsets"][int(out["delta_zero__feet"][-1, 1])])
    after, before = out["clamps__tempo_after"], out["clamps__postures"][:, 2]
    assert {0.2, 2.0} <= set((after / before).tolist())
    rows, points = out["negative_time__rule_data"], out["negative_time__points"]
    assert rows[0, 2] >= 2 and rows[0, 7] + out["intonation"][0] < 0 and points[0, 0] < points[1, 0] < points[0, 0] + 8.0
    path = os.path.join(HERE, "prosody_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
