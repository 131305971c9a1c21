// Driver of tests/golden/make_targets_golden.py: the reference's own MovingAverageFilter<float>
// (vtm/MovingAverageFilter.h, included unchanged; only its constructor, reset() and filter() are called) under the rule of
// include/gama_vtm.h, "Synthesis from parameter targets", written here as the header writes it: 16 filters of 50 ms, cur[p]
// starting at 0, steps s = 0 .. S-1, a point of list p at step s sets cur[p], and every step feeds cur[p] to filter p and
// keeps what it returns.  The editor's interactive window, whose behaviour the rule states
// (gama_tts_editor/src/interactive/InteractiveAudio.cpp:164-186), is a JACK client and cannot be built here without JACK;
// none of its text is in this file.
//
//   ref_targets_table in.bin out.bin
//   in:  "GVTI", int32 version, int32 cases; per case: double internal rate, int64 steps S; per parameter (16): int32 points,
//        points x int32 step, points x float32 value
//   out: "GVTO", int32 version, int32 cases; per case S x 16 float32
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MovingAverageFilter.h"

namespace {

template <typename T> T take(const unsigned char*& p)
{
	T v;
	std::memcpy(&v, p, sizeof v);
	p += sizeof v;
	return v;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc != 3) return 2;
	std::FILE* f = std::fopen(argv[1], "rb");
	if (!f) return 3;
	std::vector<unsigned char> in;
	unsigned char chunk[65536];
	for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) in.insert(in.end(), chunk, chunk + n);
	std::fclose(f);
	const unsigned char* p = in.data();
	if (in.size() < 12 || std::memcmp(p, "GVTI", 4) != 0) return 4;
	p += 4;
	const int32_t version = take<int32_t>(p), cases = take<int32_t>(p);
	std::FILE* out = std::fopen(argv[2], "wb");
	if (!out) return 5;
	std::fwrite("GVTO", 1, 4, out);
	std::fwrite(&version, 4, 1, out);
	std::fwrite(&cases, 4, 1, out);
	for (int32_t c = 0; c < cases; ++c) {
		const double rate = take<double>(p);
		const int64_t n_steps = take<int64_t>(p);
		std::vector<int32_t> steps[16];
		std::vector<float> values[16];
		for (int q = 0; q < 16; ++q) {
			const int32_t points = take<int32_t>(p);
			steps[q].resize(points);
			values[q].resize(points);
			for (int32_t& s : steps[q]) s = take<int32_t>(p);
			for (float& v : values[q]) v = take<float>(p);
		}
		// a fresh run: filters as the window constructs them, reset; the targets start at 0
		std::vector<GS::VTM::MovingAverageFilter<float>> filters;
		for (int q = 0; q < 16; ++q) {
			filters.emplace_back(static_cast<float>(rate), 50.0e-3);
			filters.back().reset();
		}
		float cur[16] = {};
		size_t next[16] = {};
		std::vector<float> frames(static_cast<size_t>(n_steps) * 16);
		for (int64_t s = 0; s < n_steps; ++s) {
			for (int q = 0; q < 16; ++q) {
				if (next[q] < steps[q].size() && steps[q][next[q]] == s) cur[q] = values[q][next[q]++];
				frames[static_cast<size_t>(s) * 16 + q] = filters[q].filter(cur[q]);
			}
		}
		std::fwrite(frames.data(), sizeof(float), frames.size(), out);
	}
	std::fclose(out);
	return p == in.data() + in.size() ? 0 : 6;
}
