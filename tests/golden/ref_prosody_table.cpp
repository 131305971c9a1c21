// TEST INFRASTRUCTURE — not part of the product.
//
// Drives the REAL GS::VTMControlModel::EventList through generateEventList() (with applyRhythm() at its head,
// EventList.cpp:796-819) and applyIntonation() (:687-793, :903-927) on utterances given as builder calls
// (tests/prosody_cases.py) or taken from a text through the reference's text parser and PhoneticStringParser, chunk by
// chunk as Controller::getParametersFromPhoneticString does (Controller.cpp:141-154), and records per chunk the postures
// before and after rhythm, the closed feet and tone groups, the parameter set and the draws the reference took, the rule
// data, the onsets, the IntonationPoints and the list after the merge.  Our own code, compiled against the reference where
// it lies (make_prosody_golden.py).
//
// Private access, for two things only: reading back feet_ / toneGroups_ (and the constants IntonationRhythm read from its
// files), and seeding intonationRhythm_.randSrc_ with a known seed.  A twin std::mt19937 with the same seed and the same
// distributions, run in the reference's call order -- per tone group the set index (where intonationParameters() draws
// one), per foot two reals -- records what the reference drew; if the twin is out of step the points will not match.
//
// usage: ref_prosody_table <voice_data_dir> <in.bin> <out.bin>
//   in:  "GVPI" i32 version=1; i32 n_cases, per case: i32 kind (0 calls, 1 text), i32 control_period, i32 random (0 / 1),
//        u32 seed, i32 fixed (0 / 1), f32 fixed_param[5], f32 intonation_factor, f64 global_tempo; kind 0: i32 n_calls, per
//        call i32 op (0 posture: i32 id, i32 marked, f64 tempo, f64 rule_tempo; 1 newFoot; 2 setCurrentFootMarked;
//        3 setCurrentFootTempo: f64; 4 newToneGroup; 5 setCurrentToneGroupType: i32); kind 1: i32 len, the text
//   out: "GVPO" i32 version=1; f32 intonation[8] (intonation.txt, in the order of gvtm_prosody_config), f64 rhythm[8]
//        (rhythm.txt), per tone-group type 0..4: i32 n_sets, f32 sets[n_sets][5]; i32 n_postures, u8 vocoid[n_postures];
//        i32 n_chunks, per chunk: i32 case, i32 exception (0 none, 9 one), i32 n, per posture i32 id, i32 marked, f64 tempo
//        before rhythm, f64 rule_tempo, f64 tempo after rhythm; i32 n_feet, per foot i32 start, i32 end, i32 marked, f64 tempo
//        before rhythm, f64 draws[2]; i32 n_groups, per group i32 start_foot, i32 end_foot, i32 type (6: none), f32 param[5];
//        i32 n_rules, f64 rule_data[n_rules][8]; f64 onsets[n]; i32 n_points, f64 points[n_points][3] (absoluteTime(),
//        semitone(), slope()); i32 n_events, f64 events[n_events][38] (time, has interpData, a, b, c, d, parameters[16],
//        specialParameters[16])
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#define private public
#include "EventList.h"
#include "IntonationRhythm.h"
#undef private
#include "Controller.h"
#include "Exception.h"
#include "Index.h"
#include "Model.h"
#include "PhoneticStringParser.h"
#include "TextParser.h"

namespace {

using namespace GS::VTMControlModel;

struct Reader {
	FILE* f;
	template <typename T> T get()
	{
		T v;
		if (std::fread(&v, sizeof(v), 1, f) != 1) throw std::runtime_error("short input");
		return v;
	}
	std::string text()
	{
		std::string s(static_cast<size_t>(get<std::int32_t>()), '\0');
		if (!s.empty() && std::fread(&s[0], 1, s.size(), f) != s.size()) throw std::runtime_error("short input");
		return s;
	}
};

FILE* out;
void put_i32(std::int32_t v) { std::fwrite(&v, sizeof(v), 1, out); }
void put_f32(float v) { std::fwrite(&v, sizeof(v), 1, out); }
void put_f64(double v) { std::fwrite(&v, sizeof(v), 1, out); }

struct CaseConfig {
	std::int32_t control_period, random;
	std::uint32_t seed;
	std::int32_t fixed;
	float fixed_param[5];
	float intonation_factor;
	double global_tempo;
};

std::int32_t posture_id(const Model& model, const Posture* p)
{
	for (unsigned i = 0; i < model.postureList().size(); ++i) {
		if (&model.postureList()[i] == p) return static_cast<std::int32_t>(i);
	}
	return -1;
}

// the configuration of a case on a fresh list (before the postures go in)
void configure(EventList& ev, const CaseConfig& c)
{
	ev.setUp();
	ev.setControlPeriod(c.control_period);
	ev.setMacroIntonation(true);
	ev.setSmoothIntonation(true);
	ev.setGlobalTempo(c.global_tempo);
	ev.setIntonationFactor(c.intonation_factor);
	ev.setUseFixedIntonationParameters(c.fixed != 0);
	ev.setFixedIntonationParameters(c.fixed_param[0], c.fixed_param[1], c.fixed_param[2], c.fixed_param[3], c.fixed_param[4]);
	ev.setRandomIntonation(c.random != 0);
	if (c.random) ev.intonationRhythm_.randSrc_.seed(c.seed);
}

// generateEventList(); applyIntonation() on a list that holds its postures, feet and groups; writes the chunk's record
void run_and_dump(int case_index, Model& model, EventList& ev, const CaseConfig& c)
{
	std::vector<const PostureData*> postures;
	for (unsigned i = 0;; ++i) {
		const PostureData* pd = ev.getPostureDataAtIndex(i);
		if (!pd || !pd->posture) break;
		postures.push_back(pd);
	}
	std::vector<double> tempo_before;
	for (const PostureData* pd : postures) tempo_before.push_back(pd->tempo);
	const int n_feet = ev.currentFoot_, n_groups = ev.currentToneGroup_;
	std::vector<double> foot_tempo_before;
	for (int i = 0; i < n_feet; ++i) foot_tempo_before.push_back(ev.feet_[i].tempo);

	// the twin of the reference's generator, in its call order (IntonationRhythm::intonationParameters, EventList.cpp:737-763)
	IntonationRhythm& ir = ev.intonationRhythm_;
	std::mt19937 twin(c.seed);
	std::uniform_real_distribution<> real;
	std::vector<std::array<float, 5>> group_param(static_cast<size_t>(n_groups));
	std::vector<std::array<double, 2>> draws(static_cast<size_t>(n_feet), std::array<double, 2>{0.0, 0.0});
	for (int g = 0; g < n_groups; ++g) {
		unsigned type = static_cast<unsigned>(ev.toneGroups_[g].type);
		if (type >= ir.toneGroupParameters_.size()) type = 0;
		const float* param = ir.toneGroupParameters_[type][0].data();
		if (c.fixed) {
			param = c.fixed_param;
		} else if (c.random && ir.toneGroupParameters_[type].size() > 1) {
			std::uniform_int_distribution<> index(0, static_cast<int>(ir.toneGroupParameters_[type].size()) - 1);
			param = ir.toneGroupParameters_[type][static_cast<size_t>(index(twin))].data();
		}
		std::copy(param, param + 5, group_param[static_cast<size_t>(g)].begin());
		for (int j = ev.toneGroups_[g].startFoot; c.random && j <= ev.toneGroups_[g].endFoot; ++j) {
			draws[static_cast<size_t>(j)][0] = real(twin);
			draws[static_cast<size_t>(j)][1] = real(twin);
		}
	}

	int exception = 0;
	try {
		ev.generateEventList();
		ev.applyIntonation();
	} catch (const std::exception& e) {
		std::fprintf(stderr, "case %d: %s\n", case_index, e.what());
		exception = 9;
	}
	put_i32(case_index);
	put_i32(exception);
	put_i32(static_cast<std::int32_t>(postures.size()));
	for (size_t i = 0; i < postures.size(); ++i) {
		put_i32(posture_id(model, postures[i]->posture));
		put_i32(postures[i]->marked ? 1 : 0);
		put_f64(tempo_before[i]);
		put_f64(postures[i]->ruleTempo);
		put_f64(postures[i]->tempo);
	}
	put_i32(n_feet);
	for (int i = 0; i < n_feet; ++i) {
		put_i32(ev.feet_[i].start);
		put_i32(ev.feet_[i].end);
		put_i32(ev.feet_[i].marked);
		put_f64(foot_tempo_before[static_cast<size_t>(i)]);
		put_f64(draws[static_cast<size_t>(i)][0]);
		put_f64(draws[static_cast<size_t>(i)][1]);
	}
	put_i32(n_groups);
	for (int g = 0; g < n_groups; ++g) {
		put_i32(ev.toneGroups_[g].startFoot);
		put_i32(ev.toneGroups_[g].endFoot);
		put_i32(static_cast<std::int32_t>(ev.toneGroups_[g].type));
		for (float v : group_param[static_cast<size_t>(g)]) put_f32(v);
	}
	put_i32(exception ? 0 : ev.numberOfRules());
	for (int i = 0; !exception && i < ev.numberOfRules(); ++i) {
		const RuleData& r = *ev.getRuleDataAtIndex(static_cast<unsigned>(i));
		put_f64(r.number);
		put_f64(r.firstPosture);
		put_f64(r.lastPosture);
		put_f64(r.start);
		put_f64(r.mark1);
		put_f64(r.mark2);
		put_f64(r.duration);
		put_f64(r.beat);
	}
	for (const PostureData* pd : postures) put_f64(exception ? 0.0 : pd->onset);
	put_i32(exception ? 0 : static_cast<std::int32_t>(ev.intonationPoints().size()));
	for (size_t i = 0; !exception && i < ev.intonationPoints().size(); ++i) {
		const IntonationPoint& p = ev.intonationPoints()[i];
		put_f64(p.absoluteTime());
		put_f64(p.semitone());
		put_f64(p.slope());
	}
	put_i32(exception ? 0 : static_cast<std::int32_t>(ev.list().size()));
	for (size_t i = 0; !exception && i < ev.list().size(); ++i) {
		const Event& e = *ev.list()[i];
		put_f64(e.time);
		put_f64(e.interpData ? 1.0 : 0.0);
		put_f64(e.interpData ? e.interpData->a : 0.0);
		put_f64(e.interpData ? e.interpData->b : 0.0);
		put_f64(e.interpData ? e.interpData->c : 0.0);
		put_f64(e.interpData ? e.interpData->d : 0.0);
		for (int j = 0; j < 16; ++j) put_f64(e.getParameter(j, false));
		for (int j = 0; j < 16; ++j) put_f64(e.getParameter(j, true));
	}
}

} // namespace

int main(int argc, char** argv)
{
	if (argc != 4) {
		std::fprintf(stderr, "usage: %s voice_dir in.bin out.bin\n", argv[0]);
		return 2;
	}
	try {
		const GS::Index index{argv[1]};
		FILE* in = std::fopen(argv[2], "rb");
		if (!in) { std::perror(argv[2]); return 2; }
		Reader r{in};
		char magic[4];
		if (std::fread(magic, 1, 4, in) != 4 || std::string(magic, 4) != "GVPI") throw std::runtime_error("bad magic");
		if (r.get<std::int32_t>() != 1) throw std::runtime_error("bad version");
		out = std::fopen(argv[3], "wb");
		if (!out) { std::perror(argv[3]); return 2; }
		std::fwrite("GVPO", 1, 4, out);
		put_i32(1);

		Model model;
		model.load(index);
		{
			EventList ev(index, model);
			const IntonationRhythm& ir = ev.intonationRhythm_;
			for (float v : {ir.intonationTimeOffset_, ir.pretonicBaseSlope_, ir.pretonicBaseSlopeRandom_, ir.pretonicSlopeRandomFactor_, ir.tonicBaseSlope_,
					ir.tonicContinuationBaseSlope_, ir.tonicSlopeRandomFactor_, ir.tonicSlopeOffset_}) put_f32(v);
			for (double v : {ir.rhythmMarkedA_, ir.rhythmMarkedB_, ir.rhythmMarkedDiv_, ir.rhythmUnmarkedA_, ir.rhythmUnmarkedB_, ir.rhythmUnmarkedDiv_,
					ir.rhythmMinTempo_, ir.rhythmMaxTempo_}) put_f64(v);
			for (const auto& sets : ir.toneGroupParameters_) {
				put_i32(static_cast<std::int32_t>(sets.size()));
				for (const auto& set : sets) {
					for (float v : set) put_f32(v);
				}
			}
		}
		const auto vocoid = model.findCategory("vocoid");
		if (!vocoid) throw std::runtime_error("no category vocoid");
		put_i32(static_cast<std::int32_t>(model.postureList().size()));
		for (unsigned i = 0; i < model.postureList().size(); ++i) {
			const unsigned char member = model.postureList()[i].isMemberOfCategory(*vocoid) ? 1 : 0;
			std::fwrite(&member, 1, 1, out);
		}

		const std::int32_t n_cases = r.get<std::int32_t>();
		const long chunks_at = std::ftell(out);
		put_i32(0); // the number of chunks, written at the end
		std::int32_t n_chunks = 0;
		std::unique_ptr<Controller> controller; // (only for the phonetic-string format the text cases are parsed to)
		for (std::int32_t ci = 0; ci < n_cases; ++ci) {
			const std::int32_t kind = r.get<std::int32_t>();
			CaseConfig c;
			c.control_period = r.get<std::int32_t>();
			c.random = r.get<std::int32_t>();
			c.seed = r.get<std::uint32_t>();
			c.fixed = r.get<std::int32_t>();
			for (float& v : c.fixed_param) v = r.get<float>();
			c.intonation_factor = r.get<float>();
			c.global_tempo = r.get<double>();
			EventList ev(index, model);
			if (kind == 0) {
				configure(ev, c);
				const std::int32_t n_calls = r.get<std::int32_t>();
				for (std::int32_t k = 0; k < n_calls; ++k) {
					switch (r.get<std::int32_t>()) {
					case 0: {
						const std::int32_t id = r.get<std::int32_t>(), marked = r.get<std::int32_t>();
						const double tempo = r.get<double>(), rule_tempo = r.get<double>();
						ev.newPostureWithObject(model.postureList()[static_cast<unsigned>(id)], marked != 0);
						ev.setCurrentPostureTempo(tempo);
						ev.setCurrentPostureRuleTempo(rule_tempo);
						break;
					}
					case 1: ev.newFoot(); break;
					case 2: ev.setCurrentFootMarked(); break;
					case 3: ev.setCurrentFootTempo(r.get<double>()); break;
					case 4: ev.newToneGroup(); break;
					case 5: ev.setCurrentToneGroupType(static_cast<IntonationRhythm::ToneGroup>(r.get<std::int32_t>())); break;
					default: throw std::runtime_error("unknown call");
					}
				}
				run_and_dump(ci, model, ev, c);
				++n_chunks;
			} else {
				const std::string text = r.text();
				if (!controller) controller = std::make_unique<Controller>(index, model);
				auto parser = GS::TextParser::TextParser::getInstance(index, controller->vtmControlModelConfiguration().phoStrFormat);
				const std::string pho = parser->parse(text.c_str());
				PhoneticStringParser pho_parser(index, model, ev);
				// the chunks between "/c" tokens that hold more than white space
				size_t at = pho.find("/c");
				while (at != std::string::npos) {
					const size_t next = pho.find("/c", at + 2);
					const size_t size = (next == std::string::npos ? pho.size() : next) - at;
					if (pho.find_first_not_of(" \t\r\n", at + 2) < at + size) {
						// (every chunk is seeded anew, so that each entry stands alone)
						configure(ev, c);
						pho_parser.parse(&pho[at], size);
						run_and_dump(ci, model, ev, c);
						++n_chunks;
					}
					at = next;
				}
			}
		}
		std::fseek(out, chunks_at, SEEK_SET);
		put_i32(n_chunks);
		std::fclose(in);
		if (std::fclose(out) != 0) { std::perror(argv[3]); return 2; }
	} catch (const std::exception& e) {
		std::fprintf(stderr, "exception: %s\n", e.what());
		return 1;
	}
	return 0;
}
