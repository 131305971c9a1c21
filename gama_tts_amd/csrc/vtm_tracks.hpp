// Parameter-track generation on the device: the step in front of the vocal-tract path.
// EventList::generateOutput (vtm_control_model/EventList.cpp:930-1091) for a batch of event lists.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/gama_vtm.h"
#include "vtm_design.hpp"

namespace gvtm {

struct TrackArgs {
	TrackConstants k;
	const gvtm_event* events;      // all utterances back to back
	const int64_t* event_offsets;  // [batch + 1]
	size_t batch;
	size_t max_frames;
	float* params;                 // [batch][max_frames][16]
	int32_t* frame_counts;         // [batch] or null
	gvtm_drift_state* drift;       // [batch] in/out, or null (fresh generator per utterance)
};

// A batch that mixes voices: utterance b walks its list with voice_k[voice_ids[b]] (mean and initial pitch, intonation
// flags, drift set-up and filter); k.control_period, one for the launch, is all that is read of k.  An id outside
// [0, n_voices) yields frame_counts[b] = 0 and leaves the utterance's frames and drift state untouched.
struct TrackVoicesArgs : TrackArgs {
	const TrackConstants* voice_k; // [n_voices], device memory
	const int32_t* voice_ids;      // [batch]
	int32_t n_voices;
};

// Utterances of several event lists ("chunks": Controller::getParametersFromPhoneticString runs generateOutput() once per
// /c chunk of the phonetic string, on one parameter list and with one drift generator, Controller.cpp:141-154).  Utterance
// b owns the chunks [utt_chunks[b], utt_chunks[b + 1]), chunk c the events [chunk_offsets[c], chunk_offsets[c + 1]); its
// frames are the chunks' frames one after the other, max_frames and frame_counts[b] count all of them, and drift[b] runs
// on from chunk to chunk.  event_offsets is not read.  Everything else as TrackVoicesArgs.
struct TrackChunksArgs : TrackVoicesArgs {
	const int64_t* chunk_offsets;  // [chunks + 1], device memory
	const int64_t* utt_chunks;     // [batch + 1], device memory
};

// The chunk kernel appending (an events-fed gvtm_stream): utterance b's rows [0, row_start[b]) of its block of max_frames
// rows hold frames of earlier calls, and this call's frames leave behind them, at row row_start[b] + (frame of this call).
// Nothing is written at or beyond row max_frames (a row_start outside [0, max_frames) writes nothing); frame_counts[b]
// counts the frames of this call alone.  Everything else as TrackChunksArgs.
struct TrackAppendArgs : TrackChunksArgs {
	const int32_t* row_start;      // [batch], device memory
};

// The chunk kernel on a slice of a batch whose tables are the batch's (the events-packed host entries): chunk_offsets is
// the whole batch's table and holds batch-wide event indices, utt_chunks, voice_ids, drift, frame_counts and frame_offsets
// point at the slice's first utterance, and `events` at the slice's first event, which is event `event_base` of the batch:
// chunk c's events start at events + (chunk_offsets[c] - event_base).  With `packed` the frames leave a second time, back
// to back: utterance b's at packed + (frame_offsets[b] - frame_offsets[0]) * 16, by the same 16-byte stores at every flush
// of the ring, and none at or beyond frame frame_offsets[b + 1] - frame_offsets[b] of the utterance (frame_offsets is not
// read without `packed`).  Everything else as TrackChunksArgs.
struct TrackSliceArgs : TrackChunksArgs {
	int64_t event_base;
	float* packed;                 // [frames of the slice][16], 16-byte aligned, or null
	const int64_t* frame_offsets;  // [batch + 1], device memory
};

// One launch for the five argument blocks above (instantiated for each of them in vtm_tracks.hip): ceil(batch / rows per
// wavefront) workgroups of one wavefront on `stream`; a batch of 0 launches nothing.
template <typename Args>
hipError_t launch_tracks(const Args& args, hipStream_t stream);

// What an events-fed stream keeps after a synthesis launch: in utterance b's block of max_frames rows of params, the rows
// [done[b], held[b]) move to the front.  At most kCarryMaxRows rows move (a stream keeps at most its voice's granule,
// 12 frames); an utterance with done <= 0, held <= done, held > max_frames or more rows to move is left as it is.
constexpr int kCarryMaxRows = 16;

struct CarryArgs {
	float* params;                 // [batch][max_frames][16], 16-byte aligned
	const int32_t* done;           // [batch]: rows the launch has used up
	const int32_t* held;           // [batch]: rows that held frames before it
	size_t batch;
	size_t max_frames;
};

hipError_t launch_carry_rows(const CarryArgs& args, hipStream_t stream);

} // namespace gvtm
