"""The resampler's output ranges by running remainder (csrc/vtm_design.hpp: src_bounds_at, src_bounds_step,
src_bounds_advance) against the division they replace, value for value.

Chunk c of a launch converts the output samples from Q(c) up to Q(c + 1), Q(c) = ceil((step_base + c * C) * 2^16 / time_inc).
The kernels used to divide for every chunk; now they divide once per launch (src_bounds_at) and then carry quotient and
remainder forward (src_bounds_advance with the constants of src_bounds_step).  A stand-alone host program that includes the
header the kernels include walks every chunk of every case below and compares quotient and remainder with the direct
division, and the end of a partial last chunk (with and without the 2 x pad flush zeros) with its formula:

    increments    44.1 kHz and 48 kHz out at SectionDelay 1 to 4 (internal rates 20034, 40068, 60102 and 80137 Hz), 22.05 kHz
                  out at the same four (down-sampling at SectionDelay 2 to 4: time_inc > 65536), and three the 32-bit time
                  register allows though no voice reaches them: 1, one that makes dq = 0 for every chunk length (a ratio
                  above 144), and 2^32 - 5 (remainder + dr does not fit 32 bits: the advance must not form that sum)
    chunks        32, 36, 48, 96 and 144 steps
    step_base     0, 1, C - 1, C, and odd values up to 2^33
    launches      1, 2, 7 and 30 000 chunks, the last chunk one step long, one step short, and whole

The program is built with -fsanitize=undefined,address where the compiler has those runtimes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gama_tts_amd", "csrc")
INTERNAL = (20034, 40068, 60102, 80137)  # SectionDelay 1 to 4 on the male voice's tube
OUT = (44100.0, 48000.0, 22050.0)
EXTREME = (1, 0x00A00001, 0xFFFFFFFB)
CHUNKS = (32, 36, 48, 96, 144)
LAUNCHES = (1, 2, 7, 30000)

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "vtm_design.hpp"

using namespace gvtm;

static unsigned long long checked = 0, wrong = 0;

static void expect(uint64_t got, uint64_t want, const char* what, unsigned inc, int C, uint64_t base, uint64_t c)
{
	++checked;
	if (got != want && wrong++ < 20)
		std::printf("WRONG %s inc %u C %d step_base %llu chunk %llu: %llu, the division gives %llu\n", what, inc, C,
		            (unsigned long long)base, (unsigned long long)c, (unsigned long long)got, (unsigned long long)want);
}

int main()
{
	const unsigned incs[] = {@INCS@};
	const int chunks[] = {@CHUNKS@};
	const uint64_t launches[] = {@LAUNCHES@};
	const int pad = 13;
	for (unsigned inc : incs) {
		for (int C : chunks) {
			const SrcBoundsStep st = src_bounds_step(inc, C);
			expect(st.dq, (static_cast<uint64_t>(C) << 16) / inc, "dq", inc, C, 0, 0);
			expect(st.dr, (static_cast<uint64_t>(C) << 16) % inc, "dr", inc, C, 0, 0);
			const uint64_t bases[] = {0, 1, static_cast<uint64_t>(C) - 1, static_cast<uint64_t>(C), 12345, 160ull * 999983ull, (1ull << 31) + 7,
			                          (1ull << 32) - 1, (1ull << 33) - 3, 1ull << 33};
			for (uint64_t base : bases) {
				for (uint64_t n : launches) {
					SrcBounds b = src_bounds_at(inc, base);
					for (uint64_t c = 0; c <= n; ++c) {
						const uint64_t x = ((base + c * C) << 16) + inc - 1;
						expect(b.q, x / inc, "quotient", inc, C, base, c);
						expect(b.r, x % inc, "remainder", inc, C, base, c);
						src_bounds_advance(b, st, inc);
					}
					// the last chunk's end: one step, one step short of a whole chunk, a whole chunk; a push (no flush) and a finish
					const uint64_t lasts[] = {1, static_cast<uint64_t>(C) - 1, static_cast<uint64_t>(C)};
					for (uint64_t last : lasts) {
						const uint64_t steps = (n - 1) * C + last;
						for (int flush = 0; flush < 2; ++flush) {
							const uint64_t filled = base + steps + (flush ? 2ull * pad : 0ull);
							expect(src_bounds_at(inc, filled).q, ((filled << 16) + inc - 1) / inc, "last chunk", inc, C, base, n - 1);
						}
					}
				}
			}
		}
	}
	std::printf("checked %llu wrong %llu\n", checked, wrong);
	return wrong != 0;
}
"""


def increments():
    real = sorted({int(round(65536.0 * fs / out)) for fs in INTERNAL for out in OUT})
    assert len(real) == 11 and min(real) < 65536 < max(real)  # (20034 : 22050 is 40068 : 44100)
    return real + list(EXTREME)


def test_recurrence_equals_the_division_for_every_chunk(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    src = tmp_path / "bounds.cpp"
    src.write_text(PROGRAM.replace("@INCS@", ", ".join("%du" % i for i in increments())).replace("@CHUNKS@", ", ".join(map(str, CHUNKS)))
                   .replace("@LAUNCHES@", ", ".join(map(str, LAUNCHES))))
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(tmp_path / "bounds")]
    sanitize = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if subprocess.run(base + sanitize, capture_output=True).returncode != 0:  # (a compiler without the sanitizers' runtimes)
        subprocess.run(base, check=True)
    r = subprocess.run([str(tmp_path / "bounds")], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    last = r.stdout.strip().splitlines()[-1].split()
    # 14 increments x 5 chunk lengths x 10 step_base values x (30 010 chunk boundaries, quotient and remainder each)
    assert last[0] == "checked" and int(last[1]) > 14 * 5 * 10 * 2 * 30010 and last[2:] == ["wrong", "0"]
