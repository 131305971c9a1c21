// Synthesis from parameter targets: the editor's interactive window (gama_tts_editor/src/interactive/InteractiveAudio.cpp:
// 164-186), where the user sets targets for the 16 parameters and on every internal step each parameter passes through its
// own MovingAverageFilter<float> of 50 ms into setParameter() before execSynthesisStep() runs.  No control frames, no linear
// interpolation: the parameters move on every internal sample.
//
// The rule (include/gama_vtm.h tells it in full), for N = targets_filter_length(internal rate) and per parameter a list of
// points (step, value) with strictly increasing steps: cur starts at 0; a point at step s sets cur; the filter's first call
// (step 0) fills its ring with cur and sets sum = (double)cur * (double)N; every step is sum -= leaving; sum += entering
// (moving_average_step, vtm_modification.hpp) and the parameter is (float)(sum * invN).
//
// The walk below is that rule for one parameter, the one text the host's restatement, and the synthesis kernel's
// interpolation lanes both run.  No ring: the value that leaves the window at step s is the value fed at step s - N, for
// s < N the value fed at step 0, so a second cursor through the same points, N steps behind the first, serves (the form
// vtm_modification.hpp establishes).  Built without FMA contraction (the pragma): (double)cur * N is rounded before cur is
// taken from it.  A walk may also begin in front of any later step (targets_resume: a stream's launches,
// gvtm_targets_apply_host_from), on the sum carried from the step before.
#pragma once

#include "vtm_modification.hpp"

namespace gvtm {

// what an utterance is refused for (gama_vtm.h: gvtm_targets_apply_host)
enum TargetsStatus : int32_t {
	kTargetsOk = 0,
	kTargetsBadCount = 1,   // a step count that is negative or above max_steps; device: a list id outside [0, n_lists)
	kTargetsBadOffsets = 2, // list offsets that are negative or decrease
	kTargetsBadValue = 3,   // a value that is not finite
	kTargetsBadSteps = 4,   // a negative step, steps not strictly increasing within a list
	kTargetsBadVoice = 5,   // device, several voices: a voice id outside [0, n_voices); looked at first
};

// MovingAverageFilter<float>(sampleRate, PARAMETER_FILTER_PERIOD_SEC = 50.0e-3) (InteractiveAudio.cpp:104): at 20 050 Hz the
// float product is 1002.5 and N is 1003; rounding half to even would say 1002
GVTM_HOST_DEVICE inline int64_t targets_filter_length(double internal_rate_hz)
{
	return moving_average_length(internal_rate_hz, static_cast<float>(50.0e-3));
}

constexpr int64_t kTargetsNever = INT64_MAX;

// One parameter's walk: the filter's sum, the values that enter and leave, the two cursors (the next point of each, as an
// index into the point arrays) and the steps at which they move.  The next point's step is fetched when a cursor moves, not
// when it is needed.
struct TargetsWalk {
	double sum;
	float entering, leaving;
	int64_t enter, leave, end;        // next point to enter, next point to leave, the end of the list
	int64_t next_enter, next_leave;   // the steps at which they do (kTargetsNever: the list is through)
};

// The state in front of step 0: cur is the value of a point at step 0, or 0 (paramValues_ starts at 0); the first call
// fills the ring with it.  The list is the points [first, end) of steps / values.
GVTM_HOST_DEVICE inline void targets_begin(TargetsWalk& w, const int32_t* steps, const float* values, int64_t first, int64_t end, int64_t N)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	w.entering = 0.0f;
	w.enter = first;
	w.end = end;
	if (first < end && steps[first] == 0) w.entering = values[w.enter++];
	w.leaving = w.entering;
	w.leave = w.enter;
	w.sum = static_cast<double>(w.entering) * static_cast<double>(N);
	w.next_enter = w.enter < end ? static_cast<int64_t>(steps[w.enter]) : kTargetsNever;
	w.next_leave = w.leave < end ? static_cast<int64_t>(steps[w.leave]) + N : kTargetsNever;
}

// the first point of [first, end) whose step is at or after `step` (end: none is)
GVTM_HOST_DEVICE inline int64_t targets_first_from(const int32_t* steps, int64_t first, int64_t end, int64_t step)
{
	while (first < end) {
		const int64_t mid = first + (end - first) / 2;
		if (static_cast<int64_t>(steps[mid]) < step) first = mid + 1;
		else end = mid;
	}
	return first;
}

// The state in front of step s0 > 0: the one targets_begin and s0 steps of targets_move / targets_step reach, but for the
// sum, which the caller carried (the double accumulation of floats decades apart is not exact, so it cannot be had again
// from the points).  The value that enters is the last point's before s0; the one that leaves the last point's at or before
// the window's far edge s0 - 1 - N, and with no such point the value fed at step 0.  So the list may have forgotten every
// point whose successor is at or before that edge.
GVTM_HOST_DEVICE inline void targets_resume(TargetsWalk& w, const int32_t* steps, const float* values, int64_t first, int64_t end, int64_t N, int64_t s0,
		double sum)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	w.end = end;
	w.sum = sum;
	w.enter = targets_first_from(steps, first, end, s0);
	w.entering = w.enter > first ? values[w.enter - 1] : 0.0f;
	w.leave = targets_first_from(steps, first, end, s0 - N);
	if (w.leave > first) w.leaving = values[w.leave - 1];
	else w.leaving = first < end && steps[first] == 0 ? values[first] : 0.0f;
	// (the point at step 0 left with the first call's fill: targets_begin never gives it to the leave cursor)
	if (w.leave < end && steps[w.leave] == 0) ++w.leave;
	w.next_enter = w.enter < end ? static_cast<int64_t>(steps[w.enter]) : kTargetsNever;
	w.next_leave = w.leave < end ? static_cast<int64_t>(steps[w.leave]) + N : kTargetsNever;
}

// what a list may forget in front of step s0: the first point targets_resume(.., s0, ..) and the steps behind it still
// need, which is the last one at or before the window's far edge s0 - 1 - N (the list's first where there is none)
GVTM_HOST_DEVICE inline int64_t targets_first_needed(const int32_t* steps, int64_t first, int64_t end, int64_t N, int64_t s0)
{
	const int64_t behind = targets_first_from(steps, first, end, s0 - N);
	return behind > first ? behind - 1 : first;
}

// does a cursor move at one of the steps [s, s + n)?  (No cursor is ever behind the step the walk is at.)
GVTM_HOST_DEVICE inline bool targets_moves(const TargetsWalk& w, int64_t s, int64_t n)
{
	return w.next_enter < s + n || w.next_leave < s + n;
}

// the cursors that move at step s
GVTM_HOST_DEVICE inline void targets_move(TargetsWalk& w, int64_t s, const int32_t* steps, const float* values, int64_t N)
{
	if (s == w.next_enter) {
		w.entering = values[w.enter++];
		w.next_enter = w.enter < w.end ? static_cast<int64_t>(steps[w.enter]) : kTargetsNever;
	}
	if (s == w.next_leave) {
		w.leaving = values[w.leave++];
		w.next_leave = w.leave < w.end ? static_cast<int64_t>(steps[w.leave]) + N : kTargetsNever;
	}
}

// one step behind the cursors' moves: the two additions, the multiplication, the conversion
GVTM_HOST_DEVICE inline float targets_step(TargetsWalk& w, double invN)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	w.sum = moving_average_step(w.sum, static_cast<double>(w.leaving), static_cast<double>(w.entering));
	return static_cast<float>(w.sum * invN);
}

// Per-utterance checks both sides make in the same order; the piece that looks at one point of a list that begins at `first`
GVTM_HOST_DEVICE inline bool targets_bad_step(const int32_t* steps, int64_t first, int64_t j)
{
	return steps[j] < 0 || (j > first && steps[j] <= steps[j - 1]);
}

// do utterances of `steps` internal steps fit the kernels' 31-bit step counter (with the flush behind them)?
GVTM_HOST_DEVICE inline bool targets_fits_step_counter(int64_t steps)
{
	return steps >= 0 && steps + 4096 < (int64_t(1) << 31);
}

// The host's restatement (vtm_capi_targets.cpp): the status of one utterance of n_steps steps whose parameter p owns the
// points [list_offsets[p], list_offsets[p + 1]), and with status 0 frames_out[s][p] = the parameter at step s.  A refused
// utterance leaves frames_out alone.  From first_step > 0 the walk resumes on the 16 sums of `sums`, and frames_out[0] is step
// first_step's; sums (null: not wanted, first_step 0 only) leaves as the sums after the last step.
inline int32_t targets_apply_from(int64_t N, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values, int64_t first_step,
		int64_t n_steps, double* sums, float* frames_out)
{
	if (!targets_fits_step_counter(first_step) || !targets_fits_step_counter(n_steps) || !targets_fits_step_counter(first_step + n_steps)) return kTargetsBadCount;
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		if (list_offsets[p] < 0 || list_offsets[p + 1] < list_offsets[p]) return kTargetsBadOffsets;
	}
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		for (int64_t j = list_offsets[p]; j < list_offsets[p + 1]; ++j) {
			if (!modification_finite(point_values[j])) return kTargetsBadValue;
		}
	}
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		for (int64_t j = list_offsets[p]; j < list_offsets[p + 1]; ++j) {
			if (targets_bad_step(point_steps, list_offsets[p], j)) return kTargetsBadSteps;
		}
	}
	const double invN = 1.0 / static_cast<double>(N);
	for (int p = 0; p < GVTM_N_PARAM; ++p) {
		TargetsWalk w;
		if (first_step > 0) targets_resume(w, point_steps, point_values, list_offsets[p], list_offsets[p + 1], N, first_step, sums[p]);
		else targets_begin(w, point_steps, point_values, list_offsets[p], list_offsets[p + 1], N);
		for (int64_t s = first_step; s < first_step + n_steps; ++s) {
			if (targets_moves(w, s, 1)) targets_move(w, s, point_steps, point_values, N);
			frames_out[(s - first_step) * GVTM_N_PARAM + p] = targets_step(w, invN);
		}
		if (sums) sums[p] = w.sum;
	}
	return kTargetsOk;
}

inline int32_t targets_apply(int64_t N, const int64_t* list_offsets, const int32_t* point_steps, const float* point_values, int64_t n_steps,
		float* frames_out)
{
	return targets_apply_from(N, list_offsets, point_steps, point_values, 0, n_steps, nullptr, frames_out);
}

#if defined(__HIP__)

// The check kernel's batch (vtm_kernels_targets.hip): utterance b's parameter p walks list l = list_ids ? list_ids[b][p] :
// 16 b + p, the points [list_offsets[l], list_offsets[l + 1]).  One wavefront per utterance writes the status and the
// effective step count: 0 for a refused utterance, else step_counts[b] (null: max_steps).
struct TargetsCheckArgs {
	const int64_t* list_offsets; // [n_lists + 1]
	int64_t n_lists;
	const int32_t* list_ids;     // [batch][16] or null
	const int32_t* point_steps;
	const float* point_values;
	const int32_t* step_counts;  // [batch] or null
	size_t batch, max_steps;
	int32_t* steps_out;          // [batch]
	int32_t* status;             // [batch] or null
	// several voices (gvtm_synthesize_targets_voices_device), or null: an utterance whose id is outside [0, n_voices) has
	// status kTargetsBadVoice, looked at before every other, and 0 steps (the grouping kernel leaves it out of the row map)
	const int32_t* voice_ids;    // [batch] or null
	int n_voices;
};

hipError_t launch_targets_check(const TargetsCheckArgs& args, hipStream_t stream);

#endif

} // namespace gvtm
