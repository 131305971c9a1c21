// TEST INFRASTRUCTURE — not part of the product.
//
// Runs the REAL GS::VTMControlModel::EventList through what Controller::synthesizeFromEventListToBuffer/File does to a kept
// event list (Controller.cpp:158-168, 210-224): clearMacroIntonation(), prepareMacroIntonationInterpolation()
// (EventList.cpp:822-900, 1093-1099) from a list of IntonationPoints, generateOutput() -- on event lists and points given
// as tables (tests/intonation_cases.py), and records the list the two calls leave and the frames.
// One EventList per case, set up afresh.  The points carry rule index 0: after setUp() ruleData_[0].beat is 0, so
// IntonationPoint::absoluteTime() is the offset (clamped at 0).  Only public members are used: list() hands out a const
// reference to a non-const member, so refilling it through const_cast is well defined.
// Our own code, compiled against the reference where it lies (tests/golden/make_intonation_golden.py).
//
// usage: ref_intonation_table <voice_data_dir> <in.bin> <out.bin>
//   in:  "GVII" i32 version=1, i32 n_cases; per case: i32 n_events, f64 events[n_events][38] (time, has_interp, a, b, c, d,
//        parameters[16], specialParameters[16]; +inf = not set), i32 n_points, f64 points[n_points][3] (time, semitone,
//        slope), i32 control_period, macro, micro, drift, smooth; f64 initial_pitch, mean_pitch, drift deviation, drift
//        sample rate, drift lowpass cutoff
//   out: "GVIO" i32 version=1, i32 n_cases; per case: i32 n_merged, f64 merged[n_merged][38], i32 n_frames,
//        f32 frames[n_frames][16]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <vector>

#include "EventList.h"
#include "Index.h"
#include "IntonationPoint.h"
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
void put_f64(FILE* f, double v) { std::fwrite(&v, sizeof(v), 1, f); }

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
		if (std::fread(magic, 1, 4, in) != 4 || magic[0] != 'G' || magic[1] != 'V' || magic[2] != 'I' || magic[3] != 'I') throw std::runtime_error("bad magic");
		if (r.get<std::int32_t>() != 1) throw std::runtime_error("bad version");
		const std::int32_t n_cases = r.get<std::int32_t>();

		FILE* out = std::fopen(argv[3], "wb");
		if (!out) { std::perror(argv[3]); return 2; }
		std::fwrite("GVIO", 1, 4, out);
		put_i32(out, 1);
		put_i32(out, n_cases);
		for (std::int32_t ci = 0; ci < n_cases; ++ci) {
			GS::VTMControlModel::EventList ev(index, *model);
			ev.setUp();
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
			const std::int32_t n_points = r.get<std::int32_t>();
			for (std::int32_t j = 0; j < n_points; ++j) {
				const double time = r.get<double>(), semitone = r.get<double>(), slope = r.get<double>();
				GS::VTMControlModel::IntonationPoint p(&ev);
				p.setRuleIndex(0);
				p.setOffsetTime(time);
				p.setSemitone(semitone);
				p.setSlope(slope);
				ev.intonationPoints().push_back(p);
			}
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
			ev.setUpDriftGenerator(d[2], d[3], d[4]);

			ev.clearMacroIntonation();
			ev.prepareMacroIntonationInterpolation();
			std::vector<std::vector<float>> frames;
			ev.generateOutput(frames);

			put_i32(out, static_cast<std::int32_t>(ev.list().size()));
			for (const auto& e : ev.list()) {
				put_f64(out, e->time);
				put_f64(out, e->interpData ? 1.0 : 0.0);
				put_f64(out, e->interpData ? e->interpData->a : 0.0);
				put_f64(out, e->interpData ? e->interpData->b : 0.0);
				put_f64(out, e->interpData ? e->interpData->c : 0.0);
				put_f64(out, e->interpData ? e->interpData->d : 0.0);
				for (int j = 0; j < kParams; ++j) put_f64(out, e->getParameter(j, false));
				for (int j = 0; j < kParams; ++j) put_f64(out, e->getParameter(j, true));
			}
			put_i32(out, static_cast<std::int32_t>(frames.size()));
			for (const auto& fr : frames) std::fwrite(fr.data(), sizeof(float), kParams, out);
		}
		std::fclose(in);
		if (std::fclose(out) != 0) { std::perror(argv[3]); return 2; }
	} catch (const std::exception& e) {
		std::fprintf(stderr, "exception: %s\n", e.what());
		return 1;
	}
	return 0;
}
