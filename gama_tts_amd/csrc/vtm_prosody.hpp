// Rhythm and intonation points: EventList::applyRhythm() (vtm_control_model/EventList.cpp:796-819), which runs at the head of
// generateEventList(), and EventList::applyIntonation() / addIntonationPoint() (:687-793, :903-927), which runs behind it
// and leaves the IntonationPoints that prepareMacroIntonationInterpolation() merges (vtm_intonation.hpp).  include/gama_vtm.h
// tells the rule in full; restated, not tidied.
//
// The pieces below are one text for the host entries and for the kernels (vtm_prosody.hip):
//   prosody_foot_ok / prosody_group_ok   a foot or a tone group the reference's builder could have made
//   prosody_foot_tempo                   one foot's tempo after the rhythm model
//   prosody_vocoid_posture               the posture a foot's point hangs on
//   prosody_rule_of                      the first rule row that holds a posture, searched from a row
//   prosody_pretonic / prosody_tonic / prosody_boundary   the semitone, slope and offset handed to addIntonationPoint
//   prosody_chain                        addIntonationPoint's minTime chain over an utterance's points, in order
// Floats where the reference holds floats (the tone-group parameters, intonation.txt, the intonation factor), doubles where
// it computes in double, each float widened where the C++ expression widens it; no FMA contraction (the pragmas here and
// the Makefile's flag), IEEE division.
//
// What is serial and what is not: ruleIndex is carried from foot to foot only where a posture lies in no rule
// row, which a list the rules entry accepted never has (the rows cover the postures 0 .. n - 1), so such an utterance is
// refused and every foot's lookups stand alone; offsetTime is 0 for the first foot and time_offset for every other one;
// only minTime, the stored time of the point before plus two control periods, runs through all the points in order.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/gama_vtm.h"
#include "vtm_design.hpp"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GVTM_HD __host__ __device__
#else
#define GVTM_HD
#endif

namespace gvtm {

// what an utterance is refused for (gama_vtm.h: gvtm_prosody_points_host)
enum ProsodyStatus : int32_t {
	kProsodyOk = 0,
	kProsodyBadStructure = 1, // feet, tone groups or posture ids the reference could not have built
	kProsodyNoRules = 2,      // the rules entry refused the utterance, its rule rows exceed max_rules, or a posture lies in none
	kProsodyTooMany = 3,      // more than GVTM_MAX_INTONATION_POINTS points
	kProsodyBadValue = 4,     // a tempo, draw, parameter or resulting value that is not finite
	kProsodyNoRoom = 5,       // device only: the points do not fit the output
};

constexpr int kProsodyMaxPoints = GVTM_MAX_INTONATION_POINTS;
constexpr int kProsodyToneGroupNone = 5;
constexpr int kProsodyContinuation = 3; // IntonationRhythm::ToneGroup::continuation
constexpr double kProsodyEps = 1.0e-6;  // EventList.cpp:31

GVTM_HD inline bool prosody_finite(double x) { return x - x == 0.0; }

// foot i of an utterance of n_postures: inside the postures, not empty, behind the foot in front of it
GVTM_HD inline bool prosody_foot_ok(const gvtm_foot* feet, int64_t i, int64_t n_postures)
{
	const gvtm_foot& f = feet[i];
	if (f.start < 0 || f.end < f.start || f.end >= n_postures) return false;
	return i == 0 || f.start > feet[i - 1].end;
}

// tone group g of an utterance of n_feet: inside the feet, not empty, behind the group in front of it, a type 0..5
GVTM_HD inline bool prosody_group_ok(const gvtm_tone_group* groups, int64_t g, int64_t n_feet)
{
	const gvtm_tone_group& t = groups[g];
	if (t.start_foot < 0 || t.end_foot < t.start_foot || t.end_foot >= n_feet) return false;
	if (t.type < 0 || t.type > kProsodyToneGroupNone) return false;
	return g == 0 || t.start_foot > groups[g - 1].end_foot;
}

// :799-814: the foot's tempo after the rhythm model, the clamp and the global tempo
GVTM_HD inline double prosody_foot_tempo(const gvtm_prosody_config& c, const gvtm_foot& f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const int n = f.end - f.start + 1;
	double tempo = f.tempo;
	if (f.marked) {
		const double temp = c.marked_a * n + c.marked_b;
		tempo += temp / c.marked_div;
	} else {
		const double temp = c.unmarked_a * n + c.unmarked_b;
		tempo += temp / c.unmarked_div;
	}
	if (tempo < c.min_tempo) {
		tempo = c.min_tempo;
	} else if (tempo > c.max_tempo) {
		tempo = c.max_tempo;
	}
	tempo *= c.global_tempo;
	return tempo;
}

// :719-726: the foot's first vocoid, or its first posture.  (Posture ids were checked against the table.)
GVTM_HD inline int prosody_vocoid_posture(const uint8_t* vocoid, const gvtm_posture* postures, const gvtm_foot& f)
{
	int index = f.start;
	while (!vocoid[postures[index].posture]) {
		index++;
		if (index > f.end) {
			index = f.start;
			break;
		}
	}
	return index;
}

// :728-733, :770-775: the first row from `from` on that holds the posture, or -1 (the reference would keep the row before)
GVTM_HD inline int prosody_rule_of(const gvtm_rule_data* rows, int n_rows, int from, int posture)
{
	for (int k = from; k < n_rows; k++) {
		if (posture >= rows[k].first_posture && posture <= rows[k].last_posture) return k;
	}
	return -1;
}

// what addIntonationPoint is handed, and the beat of its rule
struct ProsodyRawPoint {
	double beat, offset, semitone, slope;
};

// :712-715
GVTM_HD inline double prosody_pretonic_delta(const float* param, double start_time, double end_time)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double delta_time = end_time - start_time;
	return delta_time < kProsodyEps ? 0.0 : param[0] / delta_time;
}

// :735-749; draws: the foot's two, or null
GVTM_HD inline void prosody_pretonic(const gvtm_prosody_config& c, const float* param, const double* draws, double onset, double start_time,
		double pretonic_delta, double& semitone_out, double& slope_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	double semitone, slope;
	if (draws) {
		semitone = (draws[0] - 0.5) * param[2];
		slope = draws[1] * c.pretonic_slope_random_factor + c.pretonic_base_slope_random;
	} else {
		semitone = 0.0;
		slope = c.pretonic_base_slope;
	}
	semitone_out = (onset - start_time) * pretonic_delta + param[0] + semitone;
	slope_out = slope;
}

// :750-767
GVTM_HD inline void prosody_tonic(const gvtm_prosody_config& c, const float* param, int type, const double* draws, double& semitone_out, double& slope_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	double semitone, slope;
	if (type == kProsodyContinuation) {
		slope = c.tonic_continuation_base_slope;
	} else {
		slope = c.tonic_base_slope;
	}
	if (draws) {
		semitone = (draws[0] - 0.5) * param[4];
		slope += draws[1] * c.tonic_slope_random_factor;
	} else {
		semitone = 0.0;
		slope += c.tonic_slope_offset;
	}
	semitone_out = param[1] + param[0] + semitone; // (the first sum is a float's)
	slope_out = slope;
}

// :777-780, :786-789: the point behind a tonic foot and the closing point: a sum of three floats
GVTM_HD inline double prosody_boundary(const float* param)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	return param[1] + param[0] + param[3];
}

// IntonationPoint::absoluteTime()
GVTM_HD inline double prosody_absolute_time(double beat, double offset)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double time = beat + offset;
	return time < 0.0 ? 0.0 : time;
}

// addIntonationPoint (:903-927) over the raw points in order: the factor, then the chain through minTime.  false: a
// resulting value is not finite.
GVTM_HD inline bool prosody_chain(const gvtm_prosody_config& c, int cp, const ProsodyRawPoint* raw, int n, gvtm_intonation_point* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	bool finite = true;
	double previous = 0.0; // (no point yet: minTime = 2.0 * controlPeriod_)
	for (int i = 0; i < n; i++) {
		double offset = raw[i].offset;
		const double time = prosody_absolute_time(raw[i].beat, offset);
		const double min_time = previous + 2.0 * cp;
		if (time < min_time) offset = offset + (min_time - time);
		previous = prosody_absolute_time(raw[i].beat, offset);
		out[i].time_ms = previous;
		out[i].semitone = raw[i].semitone * c.intonation_factor;
		out[i].slope = raw[i].slope * c.intonation_factor;
		finite = finite && prosody_finite(out[i].time_ms) && prosody_finite(out[i].semitone) && prosody_finite(out[i].slope);
	}
	return finite;
}

// "" or what gvtm_prosody_create refuses
inline const char* prosody_validate(const gvtm_prosody_config& c)
{
	const double d[] = {c.marked_a, c.marked_b, c.marked_div, c.unmarked_a, c.unmarked_b, c.unmarked_div, c.min_tempo, c.max_tempo, c.global_tempo};
	for (double x : d) {
		if (!prosody_finite(x)) return "a rhythm constant or the global tempo is not finite";
	}
	const float f[] = {c.time_offset, c.pretonic_base_slope, c.pretonic_base_slope_random, c.pretonic_slope_random_factor, c.tonic_base_slope,
			c.tonic_continuation_base_slope, c.tonic_slope_random_factor, c.tonic_slope_offset, c.intonation_factor};
	for (float x : f) {
		if (!prosody_finite(x)) return "an intonation constant or the intonation factor is not finite";
	}
	return "";
}

// applyRhythm() for one utterance: postures_out (may be postures) gets the postures with their tempi multiplied.  A foot
// that is not as prosody_foot_ok wants it (status 1) or whose tempo leaves the model not finite (status 4) multiplies nothing;
// the largest status is the utterance's.  One foot at a time and no foot reads what another wrote: the kernel's lanes do the same.
inline int32_t prosody_rhythm(const gvtm_prosody_config& c, const gvtm_posture* postures, size_t n, const gvtm_foot* feet, size_t n_feet, gvtm_posture* postures_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (postures_out != postures) {
		for (size_t i = 0; i < n; ++i) postures_out[i] = postures[i];
	}
	int32_t status = kProsodyOk;
	for (size_t i = 0; i < n_feet; ++i) {
		int32_t mine = kProsodyOk;
		if (!prosody_foot_ok(feet, static_cast<int64_t>(i), static_cast<int64_t>(n))) {
			mine = kProsodyBadStructure;
		} else {
			const double tempo = prosody_foot_tempo(c, feet[i]);
			if (!prosody_finite(tempo)) {
				mine = kProsodyBadValue;
			} else {
				for (int j = feet[i].start; j < feet[i].end + 1; j++) postures_out[j].tempo *= tempo;
			}
		}
		if (mine > status) status = mine;
	}
	return status;
}

// The points the tables alone promise: feet in groups + marked feet in groups + 1, or 0 without a group; -1 for a structure
// prosody_foot_ok / prosody_group_ok refuse.
inline int64_t prosody_point_count(int64_t n_postures, const gvtm_foot* feet, int64_t n_feet, const gvtm_tone_group* groups, int64_t n_groups)
{
	for (int64_t i = 0; i < n_feet; ++i) {
		if (!prosody_foot_ok(feet, i, n_postures)) return -1;
	}
	int64_t count = 0;
	for (int64_t g = 0; g < n_groups; ++g) {
		if (!prosody_group_ok(groups, g, n_feet)) return -1;
		for (int j = groups[g].start_foot; j <= groups[g].end_foot; j++) count += feet[j].marked ? 2 : 1;
	}
	return n_groups > 0 ? count + 1 : 0;
}

// applyIntonation() up to the merge, for one utterance.  Returns the points (0 with *status != 0 for a refused utterance);
// points_out holds GVTM_MAX_INTONATION_POINTS.  rule_status: what the rules entry said of the utterance; n_rows: the rows
// it counted, of which rows[] holds min(n_rows, max_rows).  draws: two per foot, or null.
inline int prosody_points(const gvtm_prosody_config& c, const uint8_t* vocoid, int32_t n_vocoid, int cp, const gvtm_posture* postures, size_t n,
		const gvtm_foot* feet, size_t n_feet, const gvtm_tone_group* groups, size_t n_groups, const double* draws, const gvtm_rule_data* rows, size_t n_rows,
		size_t max_rows, const double* onsets, int32_t rule_status, gvtm_intonation_point* points_out, int32_t* status)
{
	*status = kProsodyOk;
	if (n > 0x7fffffffu || n_feet > 0x7fffffffu || n_groups > 0x7fffffffu) {
		*status = kProsodyBadStructure;
		return 0;
	}
	for (size_t i = 0; i < n; ++i) {
		if (postures[i].posture < 0 || postures[i].posture >= n_vocoid) {
			*status = kProsodyBadStructure;
			return 0;
		}
	}
	const int64_t count = prosody_point_count(static_cast<int64_t>(n), feet, static_cast<int64_t>(n_feet), groups, static_cast<int64_t>(n_groups));
	if (count < 0) {
		*status = kProsodyBadStructure;
		return 0;
	}
	if (rule_status != 0 || n_rows == 0 || n_rows > max_rows || n_rows > 0x7fffffffu) {
		*status = kProsodyNoRules;
		return 0;
	}
	if (n_groups == 0) return 0; // intonParms stays null
	if (count > kProsodyMaxPoints) {
		*status = kProsodyTooMany;
		return 0;
	}
	const int n_rules = static_cast<int>(n_rows);
	ProsodyRawPoint raw[kProsodyMaxPoints];
	int at = 0;
	bool first = true;
	bool finite = true;
	for (size_t g = 0; g < n_groups; ++g) {
		const gvtm_tone_group& t = groups[g];
		const double start_time = onsets[feet[t.start_foot].start];
		const double end_time = onsets[feet[t.end_foot].end];
		const double pretonic_delta = prosody_pretonic_delta(t.param, start_time, end_time);
		for (int k = 0; k < 5; ++k) finite = finite && prosody_finite(t.param[k]);
		for (int j = t.start_foot; j <= t.end_foot; j++) {
			const double* d = draws ? draws + 2 * static_cast<size_t>(j) : nullptr;
			if (d) finite = finite && prosody_finite(d[0]) && prosody_finite(d[1]);
			const int posture = prosody_vocoid_posture(vocoid, postures, feet[j]);
			const int rule = prosody_rule_of(rows, n_rules, 0, posture);
			if (rule < 0) {
				*status = kProsodyNoRules;
				return 0;
			}
			const double offset = first ? 0.0 : static_cast<double>(c.time_offset);
			first = false;
			ProsodyRawPoint& p = raw[at++];
			p.beat = rows[rule].beat;
			p.offset = offset;
			if (!feet[j].marked) {
				prosody_pretonic(c, t.param, d, onsets[posture], start_time, pretonic_delta, p.semitone, p.slope);
			} else {
				prosody_tonic(c, t.param, t.type, d, p.semitone, p.slope);
				const int rule2 = prosody_rule_of(rows, n_rules, rule, feet[j].end);
				if (rule2 < 0) {
					*status = kProsodyNoRules;
					return 0;
				}
				raw[at++] = ProsodyRawPoint{rows[rule2].beat, 0.0, prosody_boundary(t.param), 0.0};
			}
		}
	}
	raw[at++] = ProsodyRawPoint{rows[n_rules - 1].beat, 0.0, prosody_boundary(groups[n_groups - 1].param), 0.0};
	finite = prosody_chain(c, cp, raw, at, points_out) && finite;
	if (!finite) {
		*status = kProsodyBadValue;
		return 0;
	}
	return at;
}

#if defined(__HIP__)

// A batch on the device; utterance b owns the postures, feet and groups between its offsets.
struct ProsodyRhythmArgs {
	gvtm_prosody_config config;
	const gvtm_posture* postures;
	const int64_t* posture_offsets; // [batch + 1]
	int64_t n_postures;             // records behind postures and postures_out
	const gvtm_foot* feet;
	const int64_t* foot_offsets;    // [batch + 1]
	int64_t n_feet;                 // records behind feet
	size_t batch;
	gvtm_posture* postures_out;     // may be postures
	int32_t* status;                // [batch] or null
};

struct ProsodyPlaceArgs {
	gvtm_prosody_config config;
	const uint8_t* vocoid;
	int32_t n_vocoid;
	int32_t control_period;
	const gvtm_posture* postures;
	const int64_t* posture_offsets; // [batch + 1]
	const gvtm_foot* feet;
	const int64_t* foot_offsets;    // [batch + 1]
	const gvtm_tone_group* groups;
	const int64_t* group_offsets;   // [batch + 1]
	const double* draws;            // two per foot, laid out as the feet, or null
	size_t batch;
	const gvtm_rule_data* rule_data; // [batch][max_rules]
	int64_t max_rules;
	const int32_t* rule_counts;     // [batch]
	const double* onsets;           // one per posture
	gvtm_intonation_point* points_out; // [points_capacity]
	int64_t points_capacity;
	int64_t* point_offsets_out;     // [batch + 1]
	int32_t* status;                // [batch], in: the rules entry's, out: ProsodyStatus; or null
	// the prosody entry's: an utterance the rhythm kernel refused keeps that status, utterances of a voice without macro
	// intonation get no points, and list_ids_out [batch] gets b for an utterance that was not refused, -1 for one that was
	// (what gvtm_apply_intonation_device takes as list ids)
	const int32_t* rhythm_status;   // [batch] or null
	const TrackConstants* voice_k;  // [n_voices] or null
	const int32_t* voice_ids;       // [batch] or null
	int32_t n_voices;
	int32_t* list_ids_out;          // [batch] or null
};

// One kernel: a lane per foot of the batch.  A batch of 0 launches nothing.
hipError_t launch_apply_rhythm(const ProsodyRhythmArgs& args, hipStream_t stream);
// Three kernels: count (status and points per utterance), scan (lengths to offsets; points that would end beyond
// points_capacity are dropped with status 5), write.
hipError_t launch_place_intonation(const ProsodyPlaceArgs& args, hipStream_t stream);

#endif

} // namespace gvtm
