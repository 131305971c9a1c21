"""GPU-box: spectrum analysis of a resident batch (gvtm_analyze_spectrum_device) beside what a closed loop
does without it, and beside rocFFT as a yardstick.

4096 buffers of 65 536 samples (one per row: 1 GB of seeded noise on the device), Blackman window, log scale, spectrum only:
  W 65536 and W 1024, each with all 32 769 bins and with the bins up to 5 kHz (7 431 at 44.1 kHz), scratch as created
  (GVTM_ANALYSIS_DEFAULT_BUFFERS in flight), and W 65536 / all bins again with scratch for 1024 buffers
  host      the same batch as a device-to-host copy of the samples (pinned memory) plus numpy.fft.rfft, the magnitude and the
            logarithm on the host -- the copy is timed like the device variants, the transform once (it takes seconds)
  rocfft    if torch's librocfft is on the machine: torch.fft.rfft of the batch, rocFFT's batched 65 536-point real
            transform alone, with no peak, window, magnitude or logarithm -- a yardstick; the product never loads it
The device variants alternate inside every repeat; medians, wall time between HIP events after three warm-up calls each.
For each the bytes that must move (256 KB in and 4 n_bins out per buffer) over the time, and its share of 8 TB/s.  Before
anything is timed four buffers of every variant are held to the host entry and the bars of tests/analysis_cases.py.
--device-only times the device variants alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python3 tests/tools/analysis_ab.py --device-only --reps 2).
usage: python tests/tools/analysis_ab.py [--reps N] [--buffers N] [--device-only] [--out FILE.json]"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import analysis_cases as ac  # noqa: E402
import gama_tts_amd as g  # noqa: E402
from gama_tts_amd import capi  # noqa: E402
from bench_tracks_voices import timed_alternating  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12  # HBM3E, MI355X


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout.strip().splitlines()
    except (OSError, subprocess.TimeoutExpired):
        return ["rocm-smi not available"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=4096)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batch = args.buffers
    stream = torch.cuda.current_stream().cuda_stream
    generator = torch.Generator(device="cuda").manual_seed(4096)
    d_audio = torch.randn((batch, ac.N), generator=generator, dtype=torch.float32, device="cuda") * 0.25
    d_counts = torch.full((batch,), ac.N, dtype=torch.int64, device="cuda")
    results = {"buffers": batch, "reps": args.reps, "clocks_before": clocks(), "variants": {}}

    variants = [("W65536_all", 65536, 0.0, None), ("W65536_5kHz", 65536, 5000.0, None), ("W1024_all", 1024, 0.0, None),
                ("W1024_5kHz", 1024, 5000.0, None), ("W65536_all_reserve1024", 65536, 0.0, 1024)]
    fns, objects, outputs = {}, {}, {}
    sample = d_audio[:4].cpu().numpy()
    for name, W, max_freq, reserve in variants:
        an = g.Analysis(ac.BLACKMAN, W, True, -120.0, max_freq, 44100, device=0)
        if reserve:
            an.reserve(min(reserve, batch))
        d_spectra = torch.empty((batch, 1, an.n_bins), dtype=torch.float32, device="cuda")
        objects[name], outputs[name] = an, d_spectra
        fns[name] = (lambda an=an, d_spectra=d_spectra: an.analyze_device(d_audio, ac.N, d_counts, batch, 1, None, d_spectra, None, None, stream))
        # held to the host entry before anything is timed: the linear twin of the variant on four buffers
        linear = g.Analysis(ac.BLACKMAN, W, False, -120.0, max_freq, 44100, device=0)
        host = g.Analysis(ac.BLACKMAN, W, False, -120.0, max_freq, 44100, device=capi.DEVICE_NONE)
        d_linear = torch.empty((4, 1, an.n_bins), dtype=torch.float32, device="cuda")
        linear.analyze_device(d_audio, ac.N, d_counts, 4, 1, None, d_linear, None, None, stream)
        fns[name]()
        torch.cuda.synchronize()
        got, got_log, worst = d_linear.cpu().numpy(), d_spectra[:4].cpu().numpy(), 0.0
        for b in range(4):
            x = ac.prepared(sample[b], host.window())
            whole64 = ac.magnitudes64(x)
            limit, e32 = ac.bar(x, whole64)
            e = float(np.abs(got[b, 0].astype(np.float64) - whole64[: an.n_bins]).max() / whole64.max())
            assert e <= limit, (name, b, e, limit)
            worst = max(worst, e / e32)
            ac.check_log(got_log[b], got[b], -120.0)
        results["variants"][name] = {"W": W, "n_bins": an.n_bins, "reserved": reserve or capi.ANALYSIS_DEFAULT_BUFFERS,
                                     "worst_e_over_numpy_float32": worst}
        print("%s: %d bins, four buffers within the bar (worst e = %.2f of numpy float32's)" % (name, an.n_bins, worst), flush=True)

    medians, spreads = timed_alternating(fns, args.reps, 1)
    for name, ms in medians.items():
        r = results["variants"][name]
        moved = batch * (4 * ac.N + 4 * r["n_bins"])
        r.update(ms=ms, ms_min_max=spreads[name], us_per_buffer=1000.0 * ms / batch, bytes_that_must_move=moved,
                 achieved_bytes_per_s=moved / (ms * 1e-3), share_of_8TBps=moved / (ms * 1e-3) / PEAK_BYTES_PER_S)
        print("%-24s %8.3f ms (%.3f - %.3f)  %.2f us per buffer  %.1f GB/s = %.3f of peak"
              % (name, ms, spreads[name][0], spreads[name][1], r["us_per_buffer"], 1e-9 * r["achieved_bytes_per_s"], r["share_of_8TBps"]), flush=True)

    if args.device_only:
        return
    # the same batch without the entry: D2H of the samples, then numpy on the host (W 65536, all bins)
    pinned = torch.empty((batch, ac.N), dtype=torch.float32).pin_memory()
    copy_ms, copy_spread = timed_alternating({"d2h": lambda: pinned.copy_(d_audio, non_blocking=True)}, max(3, args.reps // 2), 1)
    host_audio, win = pinned.numpy(), ac.window(ac.BLACKMAN, 65536)
    t0 = time.perf_counter()
    for lo in range(0, batch, 256):
        block = host_audio[lo: lo + 256]
        peak = np.abs(block).max(axis=1, keepdims=True)
        x = ((block * (1.0 / peak.astype(np.float64)).astype(np.float32)).astype(np.float64) * win).astype(np.float32)
        mag = np.abs(np.fft.rfft(x, axis=1)) * np.float32(1.0 / 256.0)
        with np.errstate(divide="ignore"):
            np.maximum(20.0 * np.log10(mag), np.float32(-120.0))
    host_s = time.perf_counter() - t0
    results["host"] = {"d2h_ms": copy_ms["d2h"], "d2h_ms_min_max": copy_spread["d2h"], "numpy_s_once": host_s, "cpus": os.cpu_count()}
    print("host: D2H %.1f ms (%.1f GB/s), numpy normalise + window + rfft + log %.2f s (one run, one thread)"
          % (copy_ms["d2h"], 4e-9 * batch * ac.N / (copy_ms["d2h"] * 1e-3), host_s), flush=True)

    # rocFFT through torch, if torch carries it
    if glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "librocfft*")):
        try:
            ms, spread = timed_alternating({"rocfft": lambda: torch.fft.rfft(d_audio, dim=1)}, args.reps, 1)
            results["rocfft"] = {"ms": ms["rocfft"], "ms_min_max": spread["rocfft"], "us_per_buffer": 1000.0 * ms["rocfft"] / batch}
            print("rocfft (torch.fft.rfft, transform only, complex output): %.3f ms (%.3f - %.3f)" % (ms["rocfft"], *spread["rocfft"]), flush=True)
        except RuntimeError as ex:
            results["rocfft"] = {"error": str(ex).splitlines()[0]}
            print("rocfft: %s" % results["rocfft"]["error"], flush=True)
    results["clocks_after"] = clocks()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    print(json.dumps({k: v for k, v in results.items() if not k.startswith("clocks")}))


if __name__ == "__main__":
    main()
