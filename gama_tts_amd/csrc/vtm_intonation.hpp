// Intonation contours applied to event lists: what EventList holds after clearMacroIntonation() and
// prepareMacroIntonationInterpolation() (vtm_control_model/EventList.cpp:822-900, 1093-1099), the step in front of
// generateOutput() when Controller::synthesizeFromEventListToBuffer/File (Controller.cpp:158-168, 210-224) speaks a kept
// event list under a new list of IntonationPoints.
//
// The rule, for a base list of E events and P points (include/gama_vtm.h tells it in full):
//   every base event is kept bit for bit but for has_interp = 0 and interp = 0; duration = time of the last base event + 100
//   (setFullTimeScale, :679-684, before anything is inserted); point j lies at q_j = (int)max(time_ms, 0), less q_j % cp
//   (insertEvent, :302-315); a q_j no base event has becomes a new event with every parameter at +infinity; with P >= 2 the
//   event at q_j carries the polynomial of the segment to q_{j+1} (:844-883), the last one the constant (:889-897).
// The pieces both sides evaluate -- the point's place and the polynomial -- are the inline functions below, so that the
// host's restatement (vtm_design.cpp) and the device's (vtm_intonation.hip) are one text; both translation units are built
// without FMA contraction, and fp64 division is IEEE on both sides.
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

// what an utterance is refused for (gama_vtm.h: gvtm_intonation_apply_host)
enum IntonationStatus : int32_t {
	kIntonationOk = 0,
	kIntonationNoList = 1,      // empty base list, list id or voice id outside its table; host: times negative or not increasing
	kIntonationTooMany = 2,     // more than GVTM_MAX_INTONATION_POINTS points (or a negative count)
	kIntonationBadTime = 3,     // time_ms not finite or beyond duration + cp: insertEvent returns null, the reference throws
	kIntonationNotIncreasing = 4, // q_j <= q_{j-1}: the reference would divide by 0
	kIntonationNoRoom = 5,      // device only: the merged list does not fit the output
};

// Point at time_ms -> the time of its event (true), or false: insertEvent would return null (:304-309).  last_time: the
// time of the last base event.
GVTM_HD inline bool intonation_point_time(double time_ms, int cp, int last_time, int& q)
{
	q = 0;
	// (a NaN fails the first test, +-infinity the second or the third)
	if (!(time_ms == time_ms) || time_ms - time_ms != 0.0) return false;
	const double t = time_ms < 0.0 ? 0.0 : time_ms; // IntonationPoint::absoluteTime() (IntonationPoint.cpp:43-52)
	// duration + cp, in double: a list that ends within 100 ms of INT_MAX does not overflow here as the reference's int would,
	// and a time no int holds is refused like one behind the list
	if (t > static_cast<double>(last_time) + 100.0 + static_cast<double>(cp) || t >= 2147483648.0) return false;
	q = static_cast<int>(t);
	if (cp != 1) q -= q % cp;
	return true;
}

// The polynomial the event at x1 carries for the segment (x1, y1, m1) -> (x2, y2, m2): the cubic Hermite segment, or the
// straight line, that EventList.cpp:844-883 computes.  The reference writes each coefficient as one long sum of products
// and scales it by 1 / dx^3; a sum associates from the left and so does a product, so here every coefficient is a running
// sum to which the products are added or from which they are taken one at a time, in the reference's order -- the same
// roundings, one per operation.
GVTM_HD inline void intonation_segment(bool smooth, double x1, double y1, double m1, double x2, double y2, double m2, double out[4])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double dx = x2 - x1;
	if (!smooth) {
		const double rise = (y2 - y1) / dx;
		out[0] = rise;
		out[1] = y1 - x1 * rise;
		out[2] = 0.0;
		out[3] = 0.0;
		return;
	}
	const double sq1 = x1 * x1, cu1 = sq1 * x1; // powers of the segment's ends
	const double sq2 = x2 * x2, cu2 = sq2 * x2;
	const double scale = 1.0 / (dx * dx * dx);
	double s;
	// cubic term
	s = -2.0 * y2;
	s -= m1 * x1;
	s -= m2 * x1;
	s += 2.0 * y1;
	s += m1 * x2;
	s += m2 * x2;
	out[0] = s * scale;
	// square term
	s = 3.0 * y2 * x1;
	s += m1 * sq1;
	s += 2.0 * m2 * sq1;
	s -= 3.0 * x1 * y1;
	s += 3.0 * x2 * y2;
	s += m1 * x1 * x2;
	s -= m2 * x1 * x2;
	s -= 3.0 * y1 * x2;
	s -= 2.0 * m1 * sq2;
	s -= m2 * sq2;
	out[1] = s * scale;
	// linear term
	s = -(m2 * cu1);
	s -= 6.0 * y2 * x1 * x2;
	s -= 2.0 * m1 * sq1 * x2;
	s -= m2 * sq1 * x2;
	s += 6.0 * x1 * y1 * x2;
	s += m1 * x1 * sq2;
	s += 2.0 * m2 * x1 * sq2;
	s += m1 * cu2;
	out[2] = s * scale;
	// constant term
	s = -(y2 * cu1);
	s += 3.0 * y2 * sq1 * x2;
	s += m2 * cu1 * x2;
	s += m1 * sq1 * sq2;
	s -= m2 * sq1 * sq2;
	s -= 3.0 * x1 * y1 * sq2;
	s -= m1 * x1 * cu2;
	s += y1 * cu2;
	out[3] = s * scale;
}

// after the last point: constant value (:889-897)
GVTM_HD inline void intonation_last(bool smooth, double y, double out[4])
{
	out[0] = 0.0;
	out[1] = smooth ? 0.0 : y;
	out[2] = 0.0;
	out[3] = smooth ? y : 0.0;
}

// The host's restatement (vtm_design.cpp): merged events, 0 with *status != 0 for a refused utterance, or -1 if they do not
// fit `capacity`; events_out null: the count and the status alone.
int64_t intonation_apply(int control_period, bool smooth, const gvtm_event* events, size_t n_events, const gvtm_intonation_point* points,
		size_t n_points, gvtm_event* events_out, size_t capacity, int32_t* status);

#if defined(__HIP__)

// A batch on the device.  Utterance b speaks base list l = list_ids ? list_ids[b] : b, the events [list_offsets[l],
// list_offsets[l + 1]), under the points [point_offsets[b], point_offsets[b + 1]) and the configuration of its voice:
// smooth_intonation from voice_k[voice_ids[b]], the control period from `control_period` (one for the plan).
struct IntonationArgs {
	const gvtm_event* events;
	const int64_t* list_offsets;   // [n_lists + 1]
	int64_t n_lists;
	const int32_t* list_ids;       // [batch] or null
	const gvtm_intonation_point* points;
	const int64_t* point_offsets;  // [batch + 1]
	const TrackConstants* voice_k; // [n_voices], device memory
	const int32_t* voice_ids;      // [batch]
	int32_t n_voices;
	int32_t control_period;
	size_t batch;
	gvtm_event* events_out;        // [out_capacity]
	int64_t out_capacity;
	int64_t* event_offsets_out;    // [batch + 1]
	int32_t* status;               // [batch] or null
};

// Three kernels on `stream`: count (merged length and status per utterance), scan (the lengths in place to offsets; a list
// that would end beyond out_capacity gets length 0 and status 5), write.  A batch of 0 launches nothing.
hipError_t launch_apply_intonation(const IntonationArgs& args, hipStream_t stream);

#endif

} // namespace gvtm
