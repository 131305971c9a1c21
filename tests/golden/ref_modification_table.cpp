// Driver of tests/golden/make_modification_golden.py: the reference's own MovingAverageFilter<float>
// (vtm/MovingAverageFilter.h, included unchanged; only its constructor, reset() and filter() are called) under the rule of
// include/gama_vtm.h, "Parameter-modification gestures applied to frames", written here as the header writes it: frames
// k = 1 .. F-1, steps i = 0 .. cs-1 of each, s the internal step since the start; a point at step s sets cur; from the
// first point on every step feeds cur to the filter, and the first step of a frame writes the frame.  The editor's
// processor, whose behaviour the rule states (gama_tts_editor/src/ParameterModificationSynthesis.cpp:117-194), is a JACK
// client and cannot be built here without JACK; none of its text is in this file.
//
//   ref_modification_table in.bin out.bin
//   in:  "GVMI", int32 version, int32 cases; per case: double internal rate, int32 control steps, int32 frames F,
//        F x 16 float32, int32 gestures; per gesture: int32 parameter, int32 operation (0 add, 1 multiply), int32 points,
//        points x int32 step, points x float32 value
//   out: "GVMO", int32 version, int32 cases; per case F x 16 float32, the modified list after all gestures
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
	if (in.size() < 12 || std::memcmp(p, "GVMI", 4) != 0) return 4;
	p += 4;
	const int32_t version = take<int32_t>(p), cases = take<int32_t>(p);
	std::FILE* out = std::fopen(argv[2], "wb");
	if (!out) return 5;
	std::fwrite("GVMO", 1, 4, out);
	std::fwrite(&version, 4, 1, out);
	std::fwrite(&cases, 4, 1, out);
	for (int32_t c = 0; c < cases; ++c) {
		const double rate = take<double>(p);
		const int32_t cs = take<int32_t>(p);
		const int32_t frames = take<int32_t>(p);
		std::vector<float> orig(static_cast<size_t>(frames) * 16);
		for (float& v : orig) v = take<float>(p);
		std::vector<float> modified = orig;
		const int32_t gestures = take<int32_t>(p);
		for (int32_t g = 0; g < gestures; ++g) {
			const int32_t parameter = take<int32_t>(p), operation = take<int32_t>(p), points = take<int32_t>(p);
			std::vector<int32_t> steps(points);
			std::vector<float> values(points);
			for (int32_t& s : steps) s = take<int32_t>(p);
			for (float& v : values) v = take<float>(p);
			// every gesture is a fresh run: a filter as the reference constructs it, reset
			GS::VTM::MovingAverageFilter<float> average(static_cast<float>(rate), 20.0e-3);
			average.reset();
			bool have_cur = false;
			float cur = 0.0f;
			int32_t next = 0;
			for (int32_t k = 1; k < frames; ++k) {
				for (int32_t i = 0; i < cs; ++i) {
					const int64_t s = static_cast<int64_t>(k - 1) * cs + i;
					if (next < points && steps[next] == s) {
						cur = values[next++];
						have_cur = true;
					}
					if (!have_cur) continue;
					const float fm = average.filter(cur);
					if (i == 0) {
						const size_t at = static_cast<size_t>(k) * 16 + static_cast<size_t>(parameter);
						modified[at] = operation == 0 ? orig[at] + fm : orig[at] * fm;
					}
				}
			}
		}
		std::fwrite(modified.data(), sizeof(float), modified.size(), out);
	}
	std::fclose(out);
	return p == in.data() + in.size() ? 0 : 6;
}
