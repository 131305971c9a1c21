// Parameter-modification gestures applied to parameter frames: what the editor's parameter-modification window leaves in
// its modified list (gama_tts_editor ParameterModificationSynthesis.cpp:117-194, ParameterModificationWindow.cpp:200-231,
// 281-322) when the user drags one parameter while the utterance plays, and what "synthesize to file" then hands to
// Controller::synthesizeToFile.
//
// The rule, for base frames orig[F][16], the voice's control_steps (cs) and N = modification_filter_length(internal rate)
// (include/gama_vtm.h tells it in full): a gesture is one parameter, ADD or MULTIPLY, and points (step, value) with strictly
// increasing internal steps.  From the first point on, every internal step feeds the current value to a moving average of N
// floats whose sum is a double (vtm/MovingAverageFilter.h:80-92: sum -= leaving; sum += entering; two roundings, in that
// order), and at the first step of frame k >= 1 the frame takes orig[k][p] + fm or orig[k][p] * fm, fm = (float)(sum / N as
// sum * invN).  Every gesture reads orig, so a later gesture on the same parameter overwrites an earlier one from its own
// first frame on and leaves the frames before alone.
// The walk below is that rule for one gesture, the one text the host's restatement and the device's lanes both run; it is
// built without FMA contraction (the pragma and the Makefile's flag): (double)v0 * N must be rounded before v0 is taken
// from it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/gama_vtm.h"
#include "vtm_design.hpp"

// (a name of its own: vtm_math.hpp's GVTM_HD also forces inlining, and the synthesis kernels' units include both headers)
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define GVTM_HOST_DEVICE __host__ __device__
#else
#define GVTM_HOST_DEVICE
#endif

namespace gvtm {

// what an utterance is refused for (gama_vtm.h: gvtm_modification_apply_host)
enum ModificationStatus : int32_t {
	kModificationOk = 0,
	kModificationNoBase = 1,      // base or voice id outside its table, a base of fewer than 2 or more than max_frames frames
	kModificationTooMany = 2,     // more than GVTM_MAX_GESTURES gestures; device: gesture or point offsets that decrease
	kModificationBadGesture = 3,  // parameter outside [0, 16), operation other than 0 / 1, a value that is not finite
	kModificationBadSteps = 4,    // a negative step, steps not strictly increasing within a gesture
};

// MovingAverageFilter<float>(static_cast<float>(internalSampleRate()), period): buf_(std::round(sampleRate * period)), a
// float product rounded half away from zero (20 ms at 22 125 Hz: the product is 442.5 and N is 443; rounding half to even
// would say 442).  The editor has two such filters: the modification window's of 20 ms, the interactive window's of 50 ms
// (vtm_targets.hpp).
GVTM_HOST_DEVICE inline int64_t moving_average_length(double internal_rate_hz, float period)
{
	const float rate = static_cast<float>(internal_rate_hz);
	const float product = rate * period;
	return static_cast<int64_t>(static_cast<size_t>(__builtin_roundf(product)));
}

GVTM_HOST_DEVICE inline int64_t modification_filter_length(double internal_rate_hz)
{
	return moving_average_length(internal_rate_hz, static_cast<float>(20.0e-3));
}

// One call of the filter behind its first (vtm/MovingAverageFilter.h:86-88): sum -= leaving; sum += entering.  Two double
// additions, each rounded, in this order; THE text of them for both filters, host and device.
GVTM_HOST_DEVICE inline double moving_average_step(double sum, double leaving, double entering)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	sum = sum - leaving;
	sum = sum + entering;
	return sum;
}

GVTM_HOST_DEVICE inline unsigned long long modification_bits(double x)
{
	unsigned long long u;
	__builtin_memcpy(&u, &x, sizeof u);
	return u;
}

GVTM_HOST_DEVICE inline unsigned modification_bits(float x)
{
	unsigned u;
	__builtin_memcpy(&u, &x, sizeof u);
	return u;
}

GVTM_HOST_DEVICE inline bool modification_finite(float x)
{
	return (modification_bits(x) & 0x7f800000u) != 0x7f800000u;
}

// The first frame a gesture whose first point lies at `step` writes: the frame whose first internal step is the first
// multiple of cs at or behind it.  (A gesture acts if that frame exists: first < n_frames.)
GVTM_HOST_DEVICE inline int64_t modification_first_frame(int64_t step, int64_t cs)
{
	return (step + cs - 1) / cs + 1;
}

// One gesture on parameter p of a row: frames [modification_first_frame(steps[0]), min(stop_frame, n_frames)) of `out`
// take orig (+ or *) the filtered value; no other frame is touched, and the walk ends with the last of them.  orig and out
// are rows of n_frames x 16 floats and may be one row only if no other gesture reads it.
//
// No ring: the value that leaves the window at call t is the value fed at call t - N, for t < N the first value (the first
// call fills the ring with it), so a second cursor through the same points, N steps behind the first, serves.
// The shortcut: while the entering and the leaving value are the same float v, a step is sum <- RN(RN(sum - v) + v), a
// function of sum alone; once a step leaves sum as it was, every step up to the next change of either cursor does, and
// every frame up to there takes the same fm.  The walk jumps there.  A held value so costs the N steps of its entry and one.
GVTM_HOST_DEVICE inline void modification_gesture(const float* orig, float* out, int64_t n_frames, int64_t cs, int64_t N, int p, int op, const int32_t* steps,
		const float* values, int64_t n_points, int64_t stop_frame)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	constexpr int64_t kNever = INT64_MAX;
	const int64_t end_frame = stop_frame < n_frames ? stop_frame : n_frames;
	if (n_points <= 0 || end_frame < 2) return;
	const int64_t last_step = (end_frame - 2) * cs; // the step at which frame end_frame - 1 is written
	int64_t s = steps[0];
	if (s > last_step) return;
	const double invN = 1.0 / static_cast<double>(N);
	float entering = values[0], leaving = entering;
	int64_t enter = 0, leave = 0; // the points whose values enter and leave
	int64_t next_enter = n_points > 1 ? static_cast<int64_t>(steps[1]) : kNever;     // the steps at which they change
	int64_t next_leave = n_points > 1 ? static_cast<int64_t>(steps[1]) + N : kNever;
	// the first call: ring = all cur; sum = (double)cur * (double)N
	double sum = static_cast<double>(entering) * static_cast<double>(N);
	int64_t frame = modification_first_frame(s, cs); // the next frame to write, and its first step
	int64_t frame_step = (frame - 1) * cs;
	const bool add = op == GVTM_MODIFICATION_ADD;
	// Run by run: a run is the steps up to the next change of a cursor, cut where a frame begins (the frame takes the sum as
	// it is after its first step).  Inside a piece of a run nothing happens but the two additions, so the loops below are
	// those and a counter: this is the chain every lane is bound by.
	while (s <= last_step) {
		if (s == next_enter) {
			entering = values[++enter];
			next_enter = enter + 1 < n_points ? static_cast<int64_t>(steps[enter + 1]) : kNever;
		}
		if (s == next_leave) {
			leaving = values[++leave];
			next_leave = leave + 1 < n_points ? static_cast<int64_t>(steps[leave + 1]) + N : kNever;
		}
		int64_t until = next_enter < next_leave ? next_enter : next_leave; // the first step behind this run
		if (until > last_step + 1) until = last_step + 1;
		const double vin = static_cast<double>(entering), vout = static_cast<double>(leaving);
		const bool same = modification_bits(entering) == modification_bits(leaving);
		while (s < until) {
			const int64_t piece_end = frame_step < until ? frame_step + 1 : until; // (frame_step >= s throughout)
			int64_t count = piece_end - s;
			bool fixed = false;
			if (same) {
				// sum <- RN(RN(sum - v) + v): once a step leaves it as it was, every step of the run does
				for (; count > 0 && !fixed; --count) {
					const double before = sum;
					sum = moving_average_step(sum, vout, vin);
					fixed = modification_bits(sum) == modification_bits(before);
				}
			} else {
				for (; count > 0; --count) sum = moving_average_step(sum, vout, vin);
			}
			if (fixed) {
				// nothing moves before a cursor does: every frame that begins in the rest of the run takes this sum
				const float fm = static_cast<float>(sum * invN);
				for (; frame_step < until; ++frame, frame_step += cs) {
					const float o = orig[frame * GVTM_N_PARAM + p];
					out[frame * GVTM_N_PARAM + p] = add ? o + fm : o * fm;
				}
				s = until;
				break;
			}
			s = piece_end;
			if (s == frame_step + 1) {
				const float fm = static_cast<float>(sum * invN);
				const float o = orig[frame * GVTM_N_PARAM + p];
				out[frame * GVTM_N_PARAM + p] = add ? o + fm : o * fm;
				++frame;
				frame_step += cs;
			}
		}
	}
}

// Per-utterance checks both sides make in the same order; the pieces that look at one gesture or one point
GVTM_HOST_DEVICE inline bool modification_bad_gesture(int32_t parameter, int32_t operation)
{
	return parameter < 0 || parameter >= GVTM_N_PARAM || (operation != GVTM_MODIFICATION_ADD && operation != GVTM_MODIFICATION_MULTIPLY);
}

// The host's restatement (vtm_modification.hip, host side): the status of one utterance, and with status 0 frames_out =
// the frames under the gestures applied one after the other, each to the end of the utterance (the literal in-order rule;
// the device's lanes stop where a later gesture on the same parameter begins, which gives the same frames).  A refused
// utterance leaves frames_out alone.  gesture_offsets must not decrease (the caller has checked).
int32_t modification_apply(int64_t cs, int64_t N, const float* frames, size_t n_frames, const int32_t* gestures, const int64_t* gesture_offsets,
		size_t n_gestures, const int32_t* point_steps, const float* point_values, float* frames_out);

#if defined(__HIP__)

// A batch on the device.  Utterance b speaks base l = base_ids ? base_ids[b] : b, the frames base_params[l][0 .. base_frame_counts[l]),
// under the gestures [utt_gestures[b], utt_gestures[b + 1]) -- gesture g: (parameter, operation) = gestures[g][0 .. 1] and the
// points [gesture_offsets[g], gesture_offsets[g + 1]) -- with control_steps and the internal rate of voice v = voice_ids ?
// voice_ids[b] : 0 from the plan's constants on the device.
struct ModificationArgs {
	const float* base_params;          // [n_bases][max_frames][16]
	const int32_t* base_frame_counts;  // [n_bases]
	int64_t n_bases;
	const int32_t* base_ids;           // [batch] or null
	const int32_t* gestures;           // [n_gestures][2]
	const int64_t* gesture_offsets;    // [n_gestures + 1]
	const int64_t* utt_gestures;       // [batch + 1]
	const int32_t* point_steps;
	const float* point_values;
	const int32_t* voice_ids;          // [batch] or null
	const DeviceConstants* kconst;     // [n_voices], device memory
	const Model5Constants* k5const;    // [n_voices], device memory; null unless the plan is a model 5 plan
	int32_t n_voices;
	size_t batch, max_frames;
	float* params_out;                 // [batch][max_frames][16]
	int32_t* frame_counts_out;         // [batch]
	int32_t* status;                   // [batch] or null
};

// Two kernels on `stream`, one wavefront per utterance: check and copy, then the gestures.  A batch of 0 launches nothing.
hipError_t launch_apply_modifications(const ModificationArgs& args, hipStream_t stream);

#endif

} // namespace gvtm
