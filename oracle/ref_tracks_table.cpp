// TEST INFRASTRUCTURE — not part of the product.
//
// Runs the REAL GS::VTMControlModel::EventList::generateOutput() (vtm_control_model/EventList.cpp:930-1091) on event
// lists given as tables, with the settings given per call, and records the float32 frames of every call.  Where
// ref_tracks_capture takes its lists from the text parser and rules, this one takes lists the tests built to reach the
// edges of the device kernel (tests/golden/make_tracks_edges_golden.py): lengths around its LDS table, columns set far
// apart, times off the control-period grid, several events inside one period.
// One EventList per list; its calls run one after the other, so the drift generator carries over from call to call as in
// a Controller that synthesizes several chunks.  Only public members are used: list() hands out a const reference to a
// non-const member, so refilling it through const_cast is well defined.
// Our own code, compiled against the reference where it lies (oracle/Makefile target ref_full).
//
// usage: ref_tracks_table <voice_data_dir> <in.bin> <out.bin>
//   in:  "GVTI" i32 version=1, i32 n_lists; per list: i32 n_events, f64 events[n_events][38] (time, has_interp, a, b, c,
//        d, parameters[16], specialParameters[16]; +inf = not set), i32 n_calls; per call: i32 control_period, macro,
//        micro, drift, smooth; f64 initial_pitch, mean_pitch, drift deviation, drift sample rate, drift lowpass cutoff
//   out: "GVTO" i32 version=1, i32 n_lists; per list, per call: i32 n_frames, f32 frames[n_frames][16]
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <vector>

#include "EventList.h"
#include "Index.h"
#include "Model.h"

namespace {

struct Reader {
	FILE* f;
	template <typename T> T get()
	{
		T v;
		if (std::fread(&v, sizeof(v), 1, f) != 1) throw std::runtime_error("short input");
		return v;
	}
};

void put_i32(FILE* f, std::int32_t v) { std::fwrite(&v, sizeof(v), 1, f); }

constexpr int kParams = 16;
constexpr int kColumns = 6 + 2 * kParams;

} // namespace

int main(int argc, char** argv)
{
	if (argc != 4) {
		std::fprintf(stderr, "usage: %s voice_dir in.bin out.bin\n", argv[0]);
		return 2;
	}
	try {
		const GS::Index index{argv[1]};
		auto model = std::make_unique<GS::VTMControlModel::Model>();
		model->load(index);
		if (model->parameterList().size() != kParams) { std::fprintf(stderr, "expected 16 parameters\n"); return 2; }

		FILE* in = std::fopen(argv[2], "rb");
		if (!in) { std::perror(argv[2]); return 2; }
		Reader r{in};
		char magic[4];
		if (std::fread(magic, 1, 4, in) != 4 || magic[0] != 'G' || magic[1] != 'V' || magic[2] != 'T' || magic[3] != 'I') throw std::runtime_error("bad magic");
		if (r.get<std::int32_t>() != 1) throw std::runtime_error("bad version");
		const std::int32_t n_lists = r.get<std::int32_t>();

		FILE* out = std::fopen(argv[3], "wb");
		if (!out) { std::perror(argv[3]); return 2; }
		std::fwrite("GVTO", 1, 4, out);
		put_i32(out, 1);
		put_i32(out, n_lists);
		for (std::int32_t li = 0; li < n_lists; ++li) {
			GS::VTMControlModel::EventList ev(index, *model);
			auto& list = const_cast<std::vector<GS::VTMControlModel::Event_ptr>&>(ev.list());
			list.clear();
			const std::int32_t n_events = r.get<std::int32_t>();
			for (std::int32_t i = 0; i < n_events; ++i) {
				double row[kColumns];
				for (double& v : row) v = r.get<double>();
				auto e = std::make_unique<GS::VTMControlModel::Event>(kParams);
				e->time = static_cast<int>(row[0]);
				if (row[1] != 0.0) {
					e->interpData = std::make_unique<GS::VTMControlModel::InterpolationData>();
					e->interpData->a = row[2];
					e->interpData->b = row[3];
					e->interpData->c = row[4];
					e->interpData->d = row[5];
				}
				for (int j = 0; j < kParams; ++j) {
					e->setParameter(j, row[6 + j], false);
					e->setParameter(j, row[6 + kParams + j], true);
				}
				list.push_back(std::move(e));
			}
			const std::int32_t n_calls = r.get<std::int32_t>();
			for (std::int32_t c = 0; c < n_calls; ++c) {
				std::int32_t flags[5];
				for (auto& v : flags) v = r.get<std::int32_t>();
				double d[5];
				for (auto& v : d) v = r.get<double>();
				ev.setControlPeriod(flags[0]);
				ev.setMacroIntonation(flags[1] != 0);
				ev.setMicroIntonation(flags[2] != 0);
				ev.setIntonationDrift(flags[3] != 0);
				ev.setSmoothIntonation(flags[4] != 0);
				ev.setInitialPitch(d[0]);
				ev.setMeanPitch(d[1]);
				ev.setUpDriftGenerator(d[2], d[3], d[4]); // coefficients only: the generator's state runs on
				std::vector<std::vector<float>> frames;
				ev.generateOutput(frames);
				put_i32(out, static_cast<std::int32_t>(frames.size()));
				for (const auto& fr : frames) std::fwrite(fr.data(), sizeof(float), kParams, out);
			}
		}
		std::fclose(in);
		if (std::fclose(out) != 0) { std::perror(argv[3]); return 2; }
	} catch (const std::exception& e) {
		std::fprintf(stderr, "exception: %s\n", e.what());
		return 1;
	}
	return 0;
}
