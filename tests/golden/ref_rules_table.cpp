// TEST INFRASTRUCTURE — not part of the product.
//
// Drives the REAL GS::VTMControlModel::Model and EventList through generateEventList() (EventList.cpp:435-676) on posture
// sequences given as tables (tests/rules_cases.py) or taken from a text through the reference's text parser and
// PhoneticStringParser, chunk by chunk as Controller::getParametersFromPhoneticString does (Controller.cpp:141-154), and
// records per case the postures as the EventList holds them after applyRhythm(), every event (time, flag, 16 + 16 values),
// the rule data, the onsets, or which exception the reference threw.  Per model it also records the probes that pin the
// compiled arrays: every rule position's boolean expression on every posture, unmarked and marked, and every equation on
// a table of symbol vectors.  Our own code, compiled against the reference where it lies (make_rules_golden.py).
//
// usage: ref_rules_table <voice_data_dir> <in.bin> <out.bin>
//   in:  "GVRI" i32 version=1; i32 n_models, per model: i32 len, the path of its artic.xml (len 0: the voice's own);
//        i32 n_vectors, f32 vectors[n_vectors][21]; i32 n_cases, per case: i32 kind (0 table, 1 text), i32 model,
//        i32 control_period, i32 repeat (timing runs); kind 0: i32 n, per posture i32 id, i32 marked, f64 tempo,
//        f64 rule_tempo; kind 1: i32 len, the text
//   out: "GVRO" i32 version=1; per model: i32 n_rules, i32 n_postures, u8 match[n_rules][4][n_postures] (bit 0 unmarked,
//        bit 1 marked; 0 beyond the rule's positions), i32 n_equations, f32 results[n_equations][n_vectors];
//        i32 n_chunks (a table case is one chunk, a text case one per chunk of its phonetic string), per chunk: i32 case,
//        i32 exception (0 none, 1 UnavailableResourceException, 2 InvalidValueException, 9 another), i32 n, postures as
//        above, i32 n_events, f64 events[n_events][34] (time, flag, parameters[16], specialParameters[16]), i32 n_rules,
//        f64 rule_data[n_rules][8] (number, firstPosture, lastPosture, start, mark1, mark2, duration, beat), f64 onsets[n],
//        f64 nanoseconds per generateEventList() call (the mean over `repeat` runs on this machine's CPU; 0 for repeat 0)
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Controller.h"
#include "EventList.h"
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
void put_f64(double v) { std::fwrite(&v, sizeof(v), 1, out); }

struct PostureRow {
	std::int32_t id, marked;
	double tempo, rule_tempo;
};

std::int32_t posture_id(const Model& model, const Posture* p)
{
	for (unsigned i = 0; i < model.postureList().size(); ++i) {
		if (&model.postureList()[i] == p) return static_cast<std::int32_t>(i);
	}
	return -1;
}

// generateEventList() on an EventList that holds its postures; writes the chunk's record but its timing
void run_and_dump(int case_index, Model& model, EventList& ev)
{
	int exception = 0;
	try {
		ev.generateEventList();
	} catch (const GS::UnavailableResourceException&) {
		exception = 1;
	} catch (const GS::InvalidValueException&) {
		exception = 2;
	} catch (const std::exception&) {
		exception = 9;
	}
	put_i32(case_index);
	put_i32(exception);
	std::vector<const PostureData*> postures;
	for (unsigned i = 0;; ++i) {
		const PostureData* pd = ev.getPostureDataAtIndex(i);
		if (!pd || !pd->posture) break;
		postures.push_back(pd);
	}
	put_i32(static_cast<std::int32_t>(postures.size()));
	for (const PostureData* pd : postures) {
		put_i32(posture_id(model, pd->posture));
		put_i32(pd->marked ? 1 : 0);
		put_f64(pd->tempo);
		put_f64(pd->ruleTempo);
	}
	if (exception) {
		put_i32(0);
		put_i32(0);
	} else {
		put_i32(static_cast<std::int32_t>(ev.list().size()));
		for (const auto& e : ev.list()) {
			put_f64(e->time);
			put_f64(e->flag);
			for (int j = 0; j < 16; ++j) put_f64(e->getParameter(j, false));
			for (int j = 0; j < 16; ++j) put_f64(e->getParameter(j, true));
		}
		put_i32(ev.numberOfRules());
		for (int i = 0; i < ev.numberOfRules(); ++i) {
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
	}
	for (const PostureData* pd : postures) put_f64(exception ? 0.0 : pd->onset);
}

void load_postures(Model& model, EventList& ev, int control_period, const std::vector<PostureRow>& rows)
{
	ev.setUp();
	ev.setControlPeriod(control_period);
	for (const PostureRow& r : rows) {
		ev.newPostureWithObject(model.postureList()[static_cast<unsigned>(r.id)], r.marked != 0);
		ev.setCurrentPostureTempo(r.tempo);
		ev.setCurrentPostureRuleTempo(r.rule_tempo);
	}
}

double time_runs(Model& model, const GS::Index& index, int control_period, const std::vector<PostureRow>& rows, int repeat)
{
	if (repeat <= 0) return 0.0;
	EventList ev(index, model);
	double total = 0.0;
	for (int i = 0; i < repeat; ++i) {
		load_postures(model, ev, control_period, rows);
		const auto t0 = std::chrono::steady_clock::now();
		try {
			ev.generateEventList();
		} catch (const std::exception&) {
		}
		total += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
	}
	return total / repeat;
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
		if (std::fread(magic, 1, 4, in) != 4 || std::string(magic, 4) != "GVRI") throw std::runtime_error("bad magic");
		if (r.get<std::int32_t>() != 1) throw std::runtime_error("bad version");
		out = std::fopen(argv[3], "wb");
		if (!out) { std::perror(argv[3]); return 2; }
		std::fwrite("GVRO", 1, 4, out);
		put_i32(1);

		const std::int32_t n_models = r.get<std::int32_t>();
		std::vector<std::unique_ptr<Model>> models;
		for (std::int32_t i = 0; i < n_models; ++i) {
			const std::string path = r.text();
			auto model = std::make_unique<Model>();
			if (path.empty()) model->load(index);
			else model->load(path);
			if (model->parameterList().size() != 16) throw std::runtime_error("expected 16 parameters");
			models.push_back(std::move(model));
		}
		const std::int32_t n_vectors = r.get<std::int32_t>();
		std::vector<FormulaSymbolList> vectors(static_cast<size_t>(n_vectors));
		for (auto& v : vectors) {
			for (float& x : v) x = r.get<float>();
		}
		for (auto& model : models) {
			const std::int32_t n_rules = static_cast<std::int32_t>(model->ruleList().size());
			const std::int32_t n_postures = static_cast<std::int32_t>(model->postureList().size());
			put_i32(n_rules);
			put_i32(n_postures);
			for (const auto& rule : model->ruleList()) {
				for (unsigned k = 0; k < 4; ++k) {
					for (std::int32_t p = 0; p < n_postures; ++p) {
						const Posture* posture = &model->postureList()[static_cast<unsigned>(p)];
						unsigned char bits = 0;
						if (k < rule->numberOfExpressions()) {
							if (rule->evalBooleanExpression(RuleExpressionData{posture, 1.0, false}, k)) bits |= 1;
							if (rule->evalBooleanExpression(RuleExpressionData{posture, 1.0, true}, k)) bits |= 2;
						}
						std::fwrite(&bits, 1, 1, out);
					}
				}
			}
			std::int32_t n_equations = 0;
			for (const auto& group : model->equationGroupList()) n_equations += static_cast<std::int32_t>(group.equationList.size());
			put_i32(n_equations);
			for (const auto& group : model->equationGroupList()) {
				for (const auto& equation : group.equationList) {
					for (const auto& v : vectors) {
						const float y = equation->evalFormula(v);
						std::fwrite(&y, sizeof(y), 1, out);
					}
				}
			}
		}

		const std::int32_t n_cases = r.get<std::int32_t>();
		const long chunks_at = std::ftell(out);
		put_i32(0); // the number of chunks, written at the end
		std::int32_t n_chunks = 0;
		std::unique_ptr<Controller> controller; // (only for the configuration the text cases run under)
		for (std::int32_t ci = 0; ci < n_cases; ++ci) {
			const std::int32_t kind = r.get<std::int32_t>(), mi = r.get<std::int32_t>(), cp = r.get<std::int32_t>(), repeat = r.get<std::int32_t>();
			Model& model = *models.at(static_cast<size_t>(mi));
			if (kind == 0) {
				std::vector<PostureRow> rows(static_cast<size_t>(r.get<std::int32_t>()));
				for (PostureRow& row : rows) {
					row.id = r.get<std::int32_t>();
					row.marked = r.get<std::int32_t>();
					row.tempo = r.get<double>();
					row.rule_tempo = r.get<double>();
				}
				EventList ev(index, model);
				load_postures(model, ev, cp, rows);
				run_and_dump(ci, model, ev);
				put_f64(time_runs(model, index, cp, rows, repeat));
				++n_chunks;
			} else {
				const std::string text = r.text();
				if (!controller) controller = std::make_unique<Controller>(index, model);
				const auto& cfg = controller->vtmControlModelConfiguration();
				auto parser = GS::TextParser::TextParser::getInstance(index, cfg.phoStrFormat);
				const std::string pho = parser->parse(text.c_str());
				EventList ev(index, model);
				ev.setGlobalTempo(cfg.tempo);
				PhoneticStringParser pho_parser(index, model, ev);
				// the chunks between "/c" tokens that hold more than white space
				size_t at = pho.find("/c");
				while (at != std::string::npos) {
					const size_t next = pho.find("/c", at + 2);
					const size_t size = (next == std::string::npos ? pho.size() : next) - at;
					if (pho.find_first_not_of(" \t\r\n", at + 2) < at + size) {
						ev.setUp();
						ev.setControlPeriod(cp);
						pho_parser.parse(&pho[at], size);
						run_and_dump(ci, model, ev);
						// timing: the same postures, as they stand after applyRhythm(), on a fresh list
						std::vector<PostureRow> rows;
						for (unsigned i = 0;; ++i) {
							const PostureData* pd = ev.getPostureDataAtIndex(i);
							if (!pd || !pd->posture) break;
							rows.push_back(PostureRow{posture_id(model, pd->posture), pd->marked ? 1 : 0, pd->tempo, pd->ruleTempo});
						}
						put_f64(time_runs(model, index, cp, rows, repeat));
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
