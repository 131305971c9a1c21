#!/usr/bin/env python3
"""Generates tests/golden/rules_golden.npz and tests/golden/rules_model_0_male.npz by running the REAL reference (build
container only).

tests/golden/ref_rules_table.cpp is compiled here against /root/reference with the whole-library flags of oracle/Makefile
(-std=c++17 -O2 -ffp-contract=off), into a temporary directory outside the repository, and fed the cases of
tests/rules_cases.py: per case the reference's own newPostureWithObject() / tempo / rule-tempo calls (a text case: its text
parser and PhoneticStringParser, chunk by chunk) and generateEventList().  The synthetic database of rules_cases.py is
written into that directory as an artic.xml for the reference's Model to load.

rules_golden.npz holds data only:
  names                      the entries, in order (a table case by its name, a text case as <name>.<chunk>)
  <entry>__model, __cp       index into rules_cases.MODELS, control period
  <entry>__postures          [n][4] id, marked, tempo (after applyRhythm()), rule_tempo, as the reference's EventList held them
  <entry>__status            0; 1 / 2 for the reference's UnavailableResourceException / InvalidValueException; for a case the
                             reference is not run on (it would be undefined), the status the rule sets on its own
  <entry>__time, __flag      int32 [E]; __values uint64 [E][32]: the 16 + 16 values' bits
  <entry>__rule_data         [R][8] float64; __onsets float64 [n]
  <entry>__ns                nanoseconds per generateEventList() call on this machine's CPU (cases with repeat > 0)
  probe_vectors              float32 [V][21]; <model>__probe_match uint8 [rules][4][postures]; <model>__probe_equations
                             uint32 [equations][V]: the results' bits
  synthetic__<array>         the compiled arrays of the synthetic database (gama_tts_amd/control_model.py)
rules_model_0_male.npz holds the compiled arrays of data/voice/english/0_male/artic.xml and its name lists.

    python tests/golden/make_rules_golden.py
"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import rules_cases as cases  # noqa: E402
from gama_tts_amd import control_model  # noqa: E402

REF = "/root/reference"
REF_SRC = os.path.join(REF, "gama_tts", "src")
REF_VOICE_DIR = os.path.join(REF, "data", "voice", "english", "0_male")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-DENABLE_VTM_PLUGINS=1", "-DNDEBUG", "-w"]
INCLUDES = ["-I" + os.path.join(REF_SRC, d) for d in ("", "rapidxml", "text_parser", "vtm", "vtm_control_model", "xml")]
N_VECTORS = 300


def build(workdir):
    """The reference's translation units (all but main.cpp) and ref_rules_table.cpp -> workdir/ref_rules_table"""
    sources = [s for s in glob.glob(os.path.join(REF_SRC, "**", "*.cpp"), recursive=True) if os.path.basename(s) != "main.cpp"]
    objects = []
    jobs = []
    for i, src in enumerate(sorted(sources)):
        obj = os.path.join(workdir, "%03d.o" % i)
        objects.append(obj)
        jobs.append(subprocess.Popen(["g++"] + FLAGS + INCLUDES + ["-c", "-o", obj, src]))
        if len(jobs) == 8:
            assert jobs.pop(0).wait() == 0
    for j in jobs:
        assert j.wait() == 0
    exe = os.path.join(workdir, "ref_rules_table")
    subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(HERE, "ref_rules_table.cpp")] + objects + ["-ldl"], check=True)
    return exe


def probe_vectors():
    """Symbol vectors for the equation probes: plausible ones, and ones whose tempoN are small, zero or negative."""
    rng = np.random.default_rng(2024)
    v = np.empty((N_VECTORS, control_model.N_FORMULA_SYMBOLS), dtype=np.float32)
    v[:, 0:12] = rng.uniform(2.0, 400.0, (N_VECTORS, 12))
    v[:, 12:16] = rng.uniform(0.2, 3.0, (N_VECTORS, 4))
    v[:, 16:21] = rng.uniform(0.0, 600.0, (N_VECTORS, 5))
    v[200:260, 12:16] = rng.uniform(-0.01, 0.01, (60, 4))
    v[260:280, 12:16] = rng.uniform(-3.0, -0.1, (20, 4))
    v[280:290, 12:16] = 0.0
    v[290:300] = rng.normal(0.0, 1e3, (10, control_model.N_FORMULA_SYMBOLS))
    return v


def text(s):
    b = s.encode()
    return struct.pack("<i", len(b)) + b


def main():
    male = control_model.compile_model(os.path.join(REF_VOICE_DIR, "artic.xml"))
    synthetic = control_model.compile_model(cases.synthetic_xml())
    ids = {"0_male": {str(n): i for i, n in reversed(list(enumerate(male["posture_names"])))},
           "synthetic": {str(n): i for i, n in reversed(list(enumerate(synthetic["posture_names"])))}}
    vectors = probe_vectors()
    names = list(cases.CASES)
    with tempfile.TemporaryDirectory() as td:
        xml = os.path.join(td, "synthetic_artic.xml")
        with open(xml, "w") as f:
            f.write(cases.synthetic_xml())
        blob = [b"GVRI", struct.pack("<i", 1), struct.pack("<i", 2), text(""), text(xml), struct.pack("<i", N_VECTORS), vectors.astype("<f4").tobytes()]
        run = [n for n in names if cases.CASES[n]["reference"]]
        blob.append(struct.pack("<i", len(run)))
        for n in run:
            c = cases.CASES[n]
            mi = cases.MODELS.index(c["model"])
            if c["text"] is not None:
                blob.append(struct.pack("<4i", 1, mi, c["cp"], c["repeat"]) + text(c["text"]))
            else:
                blob.append(struct.pack("<4i", 0, mi, c["cp"], c["repeat"]) + struct.pack("<i", len(c["postures"])))
                for name, marked, tempo, rule_tempo in c["postures"]:
                    blob.append(struct.pack("<iidd", ids[c["model"]][name], marked, tempo, rule_tempo))
        exe = build(td)
        pin, pout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(pin, "wb") as f:
            f.write(b"".join(blob))
        subprocess.run([exe, REF_VOICE_DIR, pin, pout], check=True)
        data = open(pout, "rb").read()
    assert data[:4] == b"GVRO" and struct.unpack_from("<i", data, 4) == (1,)
    off = 8
    out = {"probe_vectors": vectors}
    for model in cases.MODELS:
        n_rules, n_postures = struct.unpack_from("<ii", data, off)
        off += 8
        out[model + "__probe_match"] = np.frombuffer(data, dtype=np.uint8, count=n_rules * 4 * n_postures, offset=off).reshape(n_rules, 4, n_postures).copy()
        off += n_rules * 4 * n_postures
        (n_equations,) = struct.unpack_from("<i", data, off)
        off += 4
        out[model + "__probe_equations"] = np.frombuffer(data, dtype="<u4", count=n_equations * N_VECTORS, offset=off).reshape(n_equations, N_VECTORS).copy()
        off += 4 * n_equations * N_VECTORS
    (n_chunks,) = struct.unpack_from("<i", data, off)
    off += 4
    entries, chunk_of = [], {}
    for _ in range(n_chunks):
        ci, exception, n = struct.unpack_from("<iii", data, off)
        off += 12
        case = run[ci]
        c = cases.CASES[case]
        if c["text"] is not None:
            entry = "%s.%d" % (case, chunk_of.get(case, 0))
            chunk_of[case] = chunk_of.get(case, 0) + 1
        else:
            entry = case
        postures = np.zeros((n, 4))
        for i in range(n):
            postures[i] = struct.unpack_from("<iidd", data, off)
            off += 24
        (n_events,) = struct.unpack_from("<i", data, off)
        off += 4
        events = np.frombuffer(data, dtype="<f8", count=n_events * 34, offset=off).reshape(n_events, 34).copy()
        off += n_events * 34 * 8
        (n_rule_rows,) = struct.unpack_from("<i", data, off)
        off += 4
        rule_data = np.frombuffer(data, dtype="<f8", count=n_rule_rows * 8, offset=off).reshape(n_rule_rows, 8).copy()
        off += n_rule_rows * 64
        onsets = np.frombuffer(data, dtype="<f8", count=n, offset=off).copy()
        off += 8 * n
        (ns,) = struct.unpack_from("<d", data, off)
        off += 8
        assert exception in (0, 1, 2), (entry, exception)
        entries.append(entry)
        out[entry + "__model"] = np.int32(cases.MODELS.index(c["model"]))
        out[entry + "__cp"] = np.int32(c["cp"])
        out[entry + "__postures"] = postures
        out[entry + "__status"] = np.int32(exception)
        out[entry + "__time"] = events[:, 0].astype(np.int32)
        out[entry + "__flag"] = events[:, 1].astype(np.int32)
        out[entry + "__values"] = np.ascontiguousarray(events[:, 2:]).view(np.uint64)
        out[entry + "__rule_data"] = rule_data
        out[entry + "__onsets"] = onsets
        if c["repeat"]:
            out[entry + "__ns"] = np.float64(ns)
        print(entry, "status", exception, n, "postures", n_events, "events", n_rule_rows, "rules", ("%.0f ns" % ns) if c["repeat"] else "")
    assert off == len(data)
    # the cases the reference is not asked about, with the status the rule sets on its own, in the cases' order
    order = []
    for n in names:
        c = cases.CASES[n]
        if c["reference"]:
            order += [e for e in entries if e == n or e.split(".")[0] == n and c["text"] is not None]
            continue
        rows = np.array([[ids[c["model"]].get(p[0], p[0]) if isinstance(p[0], str) else p[0], p[1], p[2], p[3]] for p in c["postures"]], dtype=np.float64)
        out[n + "__model"] = np.int32(cases.MODELS.index(c["model"]))
        out[n + "__cp"] = np.int32(c["cp"])
        out[n + "__postures"] = rows
        out[n + "__status"] = np.int32(cases.OWN_STATUS[n])
        out[n + "__time"] = np.zeros(0, np.int32)
        out[n + "__flag"] = np.zeros(0, np.int32)
        out[n + "__values"] = np.zeros((0, 32), np.uint64)
        out[n + "__rule_data"] = np.zeros((0, 8))
        out[n + "__onsets"] = np.zeros(rows.shape[0])
        order.append(n)
    out["names"] = np.asarray(order)
    for k in control_model.ARRAYS:
        out["synthetic__" + k] = synthetic[k]
    out["synthetic__posture_names"] = synthetic["posture_names"]
    path = os.path.join(HERE, "rules_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "rules_model_0_male.npz")
    np.savez_compressed(path, **male)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
