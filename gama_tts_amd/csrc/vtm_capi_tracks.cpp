// C ABI of libgama_vtm.so, event lists on the device: the frame counts of the host's walk, track generation, the
// events entries, which put a synthesis launch behind the tracks kernel with a frame buffer of the plan's in between, and
// the intonation entries, which put the contour's events and polynomials into the lists in front of all that.
#include "vtm_host.hpp"
#include "vtm_intonation.hpp"

using namespace gvtm::host;

namespace {

// The event lists of a batch that mixes voices: one list per utterance (d_offsets [batch + 1], the events-voices entries) or
// several (chunked: d_offsets the chunks' event offsets, d_utt_chunks [batch + 1] the utterances' chunks)
struct VoiceEvents {
	const gvtm_event* d_events;
	const int64_t* d_offsets;
	const int32_t* d_voice_ids;
	bool chunked = false;
	const int64_t* d_utt_chunks = nullptr;
};

// What the events-voices and events-chunks entries share up to the tracks launch: the checks in the order the header gives
// them, then the voice or the chunk variant of the tracks kernel on the caller's stream.
int launch_voice_tracks(gvtm_plan* plan, const VoiceEvents& lists, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream)
{
	if (batch == 0) return GVTM_OK;
	if (!lists.d_events || !lists.d_offsets || !lists.d_voice_ids) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events, offsets or voice ids");
	if (lists.chunked && !lists.d_utt_chunks) return fail(GVTM_ERR_INVALID_ARGUMENT, "null utt_chunks");
	if (!d_params && max_frames > 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null params with max_frames > 0");
	// frames leave the kernel as float4 stores
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	gvtm::TrackChunksArgs args = plan_track_args(plan, lists.d_events, lists.d_voice_ids, batch, max_frames, d_params, d_frame_counts, d_drift);
	(lists.chunked ? args.chunk_offsets : args.event_offsets) = lists.d_offsets;
	args.utt_chunks = lists.d_utt_chunks; // (null unless chunked)
	const hipError_t e = lists.chunked ? gvtm::launch_tracks<gvtm::TrackChunksArgs>(args, static_cast<hipStream_t>(hip_stream))
	                                   : gvtm::launch_tracks<gvtm::TrackVoicesArgs>(args, static_cast<hipStream_t>(hip_stream));
	if (e != hipSuccess) return fail_hip(e, lists.chunked ? "track generation launch (chunks)" : "track generation launch (voices)");
	return GVTM_OK;
}

// null plan, no table yet, design-only plan: in this order (a design-only plan still tells whether its table is set)
int check_voice_tracks_plan(const gvtm_plan* plan, const char* entry)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, std::string(entry) + ": the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	return GVTM_OK;
}

int generate_voice_tracks(gvtm_plan* plan, const char* entry, const VoiceEvents& lists, size_t batch, size_t max_frames, float* d_params,
		int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream)
{
	int rc = check_voice_tracks_plan(plan, entry);
	if (rc != GVTM_OK) return rc;
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	return launch_voice_tracks(plan, lists, batch, max_frames, d_params, d_frame_counts, d_drift, hip_stream);
}

int synthesize_voice_events(gvtm_plan* plan, const char* entry, const VoiceEvents& lists, size_t batch, size_t max_frames, float* d_audio,
		size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream)
{
	int rc = check_voice_tracks_plan(plan, entry);
	if (rc != GVTM_OK) return rc;
	if (batch == 0) return GVTM_OK;
	// (what the synthesis launch would refuse is refused before the tracks kernel advances the drift states)
	if (!d_audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if ((rc = check_audio_stride(plan, audio_stride, max_frames, true)) != GVTM_OK) return rc;
	// As gvtm_synthesize_events_device: two launches on the caller's stream with the plan's frame buffer in between; the
	// frame counts of the tracks kernel (0 for a bad voice id, which the grouping kernel fails on its own) are the
	// synthesis launch's.
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	float* frames;
	int32_t* counts;
	if ((rc = events_scratch(plan, batch, max_frames, d_frame_counts, frames, counts)) != GVTM_OK) return rc;
	if ((rc = launch_voice_tracks(plan, lists, batch, max_frames, frames, counts, d_drift, hip_stream)) != GVTM_OK) return rc;
	return launch_synthesis(plan, LaunchRequest{frames, counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream, 0, true,
			lists.d_voice_ids, &plan->async.groups});
}

// The batch of an intonation entry as the caller gives it
struct IntonationLists {
	const gvtm_event* d_events;
	const int64_t* d_list_offsets;
	size_t n_lists;
	const int32_t* d_list_ids;
	const gvtm_intonation_point* d_points;
	const int64_t* d_point_offsets;
	const int32_t* d_voice_ids;
};

// What the two intonation entries refuse before any device work, in the order the header gives; GVTM_OK with batch == 0 is
// the caller's to return.  null_output: the apply entry's own outputs, one of which is null.
int check_intonation(const gvtm_plan* plan, const char* entry, const IntonationLists& in, size_t batch, bool null_output = false)
{
	if (!plan) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan");
	if (plan->voice_tracks.empty()) return fail(GVTM_ERR_INVALID_ARGUMENT, std::string(entry) + ": the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	if (batch > 0) {
		if (!in.d_events || !in.d_list_offsets || !in.d_points || !in.d_point_offsets || !in.d_voice_ids) {
			return fail(GVTM_ERR_INVALID_ARGUMENT, "null events, list offsets, points, point offsets or voice ids");
		}
		if (null_output) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events_out or event_offsets_out");
		if (!in.d_list_ids && in.n_lists != batch) return fail(GVTM_ERR_INVALID_ARGUMENT, "without list ids every utterance has a list of its own: n_lists must equal batch");
		if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	}
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	return GVTM_OK;
}

// the three apply kernels on the caller's stream (the plan's device is current)
int launch_intonation(gvtm_plan* plan, const IntonationLists& in, size_t batch, gvtm_event* d_events_out, size_t out_capacity, int64_t* d_event_offsets_out,
		int32_t* d_status, void* hip_stream)
{
	gvtm::IntonationArgs args{};
	args.events = in.d_events;
	args.list_offsets = in.d_list_offsets;
	args.n_lists = static_cast<int64_t>(std::min<size_t>(in.n_lists, INT64_MAX));
	args.list_ids = in.d_list_ids;
	args.points = in.d_points;
	args.point_offsets = in.d_point_offsets;
	args.voice_k = static_cast<const gvtm::TrackConstants*>(plan->d_voice_tracks.ptr);
	args.voice_ids = in.d_voice_ids;
	args.n_voices = plan->n_voices();
	args.control_period = plan->voice_tracks[0].control_period;
	args.batch = batch;
	args.events_out = d_events_out;
	args.out_capacity = static_cast<int64_t>(std::min<size_t>(out_capacity, INT64_MAX));
	args.event_offsets_out = d_event_offsets_out;
	args.status = d_status;
	const hipError_t e = gvtm::launch_apply_intonation(args, static_cast<hipStream_t>(hip_stream));
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "intonation launch");
}

} // namespace

extern "C" {

int64_t gvtm_intonation_apply_host(const gvtm_track_config* config, const gvtm_event* events, size_t n_events, const gvtm_intonation_point* points,
		size_t n_points, gvtm_event* events_out, size_t capacity, int32_t* status_out)
{
	if (!config || !status_out || (!events && n_events > 0) || (!points && n_points > 0)) { fail(GVTM_ERR_INVALID_ARGUMENT, "null config, status, events or points"); return -1; }
	gvtm::TrackConstants k;
	const char* why = gvtm::design_tracks(*config, k);
	if (why[0]) { fail(GVTM_ERR_INVALID_ARGUMENT, why); return -1; }
	const int64_t merged = gvtm::intonation_apply(k.control_period, k.smooth_intonation != 0, events, n_events, points, n_points, events_out, capacity, status_out);
	if (merged < 0) fail(GVTM_ERR_INVALID_ARGUMENT, "the merged list does not fit capacity (at most n_events + n_points events)");
	return merged;
}

int gvtm_apply_intonation_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const gvtm_intonation_point* d_points, const int64_t* d_point_offsets, const int32_t* d_voice_ids, size_t batch, gvtm_event* d_events_out,
		size_t out_capacity, int64_t* d_event_offsets_out, int32_t* d_status, void* hip_stream)
{
	const IntonationLists in{d_events, d_list_offsets, n_lists, d_list_ids, d_points, d_point_offsets, d_voice_ids};
	int rc = check_intonation(plan, "gvtm_apply_intonation_device", in, batch, !d_events_out || !d_event_offsets_out);
	if (rc != GVTM_OK || batch == 0) return rc;
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	return launch_intonation(plan, in, batch, d_events_out, out_capacity, d_event_offsets_out, d_status, hip_stream);
}

int gvtm_synthesize_intonation_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_list_offsets, size_t n_lists, const int32_t* d_list_ids,
		const gvtm_intonation_point* d_points, const int64_t* d_point_offsets, const int32_t* d_voice_ids, size_t events_capacity, size_t batch,
		size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift,
		int32_t* d_status, void* hip_stream)
{
	const IntonationLists in{d_events, d_list_offsets, n_lists, d_list_ids, d_points, d_point_offsets, d_voice_ids};
	int rc = check_intonation(plan, "gvtm_synthesize_intonation_device", in, batch);
	if (rc != GVTM_OK || batch == 0) return rc;
	// (what the synthesis launch would refuse is refused before the apply kernels write a status)
	if (!d_audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if ((rc = check_audio_stride(plan, audio_stride, max_frames, true)) != GVTM_OK) return rc;
	if (events_capacity > SIZE_MAX / sizeof(gvtm_event)) return fail(GVTM_ERR_INVALID_ARGUMENT, "events_capacity too large");
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	hipError_t e;
	// (the events' pointer goes to the kernels even when there is room for none)
	if ((e = plan->async.events.ensure(sizeof(gvtm_event) * std::max<size_t>(events_capacity, 1))) != hipSuccess) return fail_hip(e, "hipMalloc merged events");
	if ((e = plan->async.event_offsets.ensure(sizeof(int64_t) * (batch + 1))) != hipSuccess) return fail_hip(e, "hipMalloc merged event offsets");
	gvtm_event* merged = plan->async.events.as<gvtm_event>();
	int64_t* offsets = plan->async.event_offsets.as<int64_t>();
	if ((rc = launch_intonation(plan, in, batch, merged, events_capacity, offsets, d_status, hip_stream)) != GVTM_OK) return rc;
	return synthesize_voice_events(plan, "gvtm_synthesize_intonation_device", VoiceEvents{merged, offsets, d_voice_ids}, batch, max_frames, d_audio,
			audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift, hip_stream);
}

size_t gvtm_tracks_frame_count(const gvtm_track_config* config, const gvtm_event* events, size_t n_events)
{
	if (!config || (!events && n_events > 0)) { fail(GVTM_ERR_INVALID_ARGUMENT, "null config or events"); return static_cast<size_t>(-1); }
	gvtm::TrackConstants k;
	const char* why = gvtm::design_tracks(*config, k);
	if (why[0]) { fail(GVTM_ERR_INVALID_ARGUMENT, why); return static_cast<size_t>(-1); }
	return gvtm::tracks_frame_count(k.control_period, events, n_events);
}

size_t gvtm_tracks_chunks_frame_count(const gvtm_track_config* config, const gvtm_event* events, const int64_t* chunk_offsets, size_t n_chunks)
{
	if (!config || (n_chunks > 0 && (!events || !chunk_offsets))) { fail(GVTM_ERR_INVALID_ARGUMENT, "null config, events or chunk_offsets"); return static_cast<size_t>(-1); }
	gvtm::TrackConstants k;
	const char* why = gvtm::design_tracks(*config, k);
	if (why[0]) { fail(GVTM_ERR_INVALID_ARGUMENT, why); return static_cast<size_t>(-1); }
	if (check_offsets(chunk_offsets, n_chunks, "chunk_offsets", FirstOffset::kNotBelowZero) != GVTM_OK) return static_cast<size_t>(-1);
	return chunks_frame_count(k.control_period, events, chunk_offsets, 0, static_cast<int64_t>(n_chunks));
}

int gvtm_generate_tracks_device(int device, const gvtm_track_config* config, const gvtm_event* d_events,
		const int64_t* d_event_offsets, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts,
		gvtm_drift_state* d_drift, void* hip_stream)
{
	if (!config || !d_event_offsets || (!d_params && max_frames > 0)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null argument");
	gvtm::TrackArgs args{};
	const char* why = gvtm::design_tracks(*config, args.k);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, why);
	if (batch == 0) return GVTM_OK;
	if (!d_events) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events");
	// frames leave the kernel as float4 stores
	if (reinterpret_cast<uintptr_t>(d_params) & 15) return fail(GVTM_ERR_INVALID_ARGUMENT, "d_params must be 16-byte aligned");
	if (const int rc = check_device_index(device, "track generation"); rc != GVTM_OK) return rc;
	DeviceScope scope(device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	args.events = d_events;
	args.event_offsets = d_event_offsets;
	args.batch = batch;
	args.max_frames = max_frames;
	args.params = d_params;
	args.frame_counts = d_frame_counts;
	args.drift = d_drift;
	const hipError_t e = gvtm::launch_tracks(args, static_cast<hipStream_t>(hip_stream));
	if (e != hipSuccess) return fail_hip(e, "track generation launch");
	return GVTM_OK;
}

int gvtm_generate_tracks_host(int device, const gvtm_track_config* config, const gvtm_event* events,
		const int64_t* event_offsets, size_t batch, size_t max_frames, float* params, int32_t* frame_counts,
		gvtm_drift_state* drift)
{
	if (!config || !event_offsets || (!params && max_frames > 0)) return fail(GVTM_ERR_INVALID_ARGUMENT, "null argument");
	if (batch == 0) return GVTM_OK;
	if (!events) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events");
	int rc = check_offsets(event_offsets, batch, "event_offsets", FirstOffset::kZero);
	if (rc == GVTM_OK) rc = check_device_index(device, "track generation");
	if (rc != GVTM_OK) return rc;
	DeviceScope scope(device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	hipError_t e;
	const size_t n_events = static_cast<size_t>(event_offsets[batch]);
	DeviceBuffer d_ev, d_off, d_par, d_cnt, d_dr;
	// (the events' and the frames' pointers go to the kernel even when there are none of either)
	if ((rc = upload(d_ev, events, n_events, "upload events", 1)) != GVTM_OK) return rc;
	if ((rc = upload(d_off, event_offsets, batch + 1, "upload event offsets")) != GVTM_OK) return rc;
	if (drift && (rc = upload(d_dr, drift, batch, "upload drift states")) != GVTM_OK) return rc;
	if ((e = d_par.ensure(sizeof(float) * 16 * std::max<size_t>(batch * max_frames, 1))) != hipSuccess) return fail_hip(e, "hipMalloc frames");
	if ((e = d_cnt.ensure(sizeof(int32_t) * batch)) != hipSuccess) return fail_hip(e, "hipMalloc frame counts");
	if ((e = hipMemset(d_par.ptr, 0, sizeof(float) * 16 * batch * max_frames)) != hipSuccess) return fail_hip(e, "hipMemset");
	rc = gvtm_generate_tracks_device(device, config, d_ev.as<gvtm_event>(), d_off.as<int64_t>(), batch, max_frames, d_par.as<float>(), d_cnt.as<int32_t>(),
			drift ? d_dr.as<gvtm_drift_state>() : nullptr, nullptr);
	if (rc != GVTM_OK) return rc;
	if ((e = hipDeviceSynchronize()) != hipSuccess) return fail_hip(e, "track generation kernel");
	if (params && (rc = download(params, d_par, 16 * batch * max_frames, "D2H frames")) != GVTM_OK) return rc;
	if (frame_counts && (rc = download(frame_counts, d_cnt, batch, "D2H counts")) != GVTM_OK) return rc;
	return drift ? download(drift, d_dr, batch, "D2H drift") : GVTM_OK;
}

int gvtm_synthesize_events_device(gvtm_plan* plan, const gvtm_track_config* config, const gvtm_event* d_events,
		const int64_t* d_event_offsets, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride,
		int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream)
{
	if (!plan || !config) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan or config");
	if (plan->n_voices() > 1) return refuse_voices(plan, "gvtm_synthesize_events_device");
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (batch == 0) return GVTM_OK;
	if (!d_events || !d_event_offsets) return fail(GVTM_ERR_INVALID_ARGUMENT, "null events or event_offsets");
	gvtm::TrackConstants tk{};
	const char* why = gvtm::design_tracks(*config, tk);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, why);
	if (!control_period_matches(plan, tk)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period_ms of the track configuration and the plan's control rate disagree");
	}
	// Two launches on the caller's stream with a frame buffer of the plan's in between.  (Walking the event lists inside the
	// synthesis kernel's interpolation wavefront was built and measured: bit-identical, no frame buffer, and 17.2 -> 33.1 ms
	// per 4096 x 80 events -- an event boundary is a round trip to memory in the middle of a tick, three times over because
	// the parameter groups run at different lags -- and 125 ms with the next events prefetched into registers, which that
	// wavefront does not have to spare.  DESIGN.md 6b.)
	DeviceScope scope(plan->device);
	int rc = scope.entered();
	if (rc != GVTM_OK) return rc;
	float* frames;
	int32_t* counts;
	rc = events_scratch(plan, batch, max_frames, d_frame_counts, frames, counts);
	if (rc == GVTM_OK) rc = gvtm_generate_tracks_device(plan->device, config, d_events, d_event_offsets, batch, max_frames, frames, counts, d_drift, hip_stream);
	if (rc != GVTM_OK) return rc;
	return launch_synthesis(plan, LaunchRequest{frames, counts, batch, max_frames, d_audio, audio_stride, d_out_counts, d_maxabs, hip_stream});
}

int gvtm_generate_tracks_voices_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_event_offsets, const int32_t* d_voice_ids,
		size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift, void* hip_stream)
{
	return generate_voice_tracks(plan, "gvtm_generate_tracks_voices_device", VoiceEvents{d_events, d_event_offsets, d_voice_ids}, batch, max_frames,
			d_params, d_frame_counts, d_drift, hip_stream);
}

int gvtm_synthesize_events_voices_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_event_offsets, const int32_t* d_voice_ids,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs,
		gvtm_drift_state* d_drift, void* hip_stream)
{
	return synthesize_voice_events(plan, "gvtm_synthesize_events_voices_device", VoiceEvents{d_events, d_event_offsets, d_voice_ids}, batch, max_frames,
			d_audio, audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift, hip_stream);
}

int gvtm_generate_tracks_chunks_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_params, int32_t* d_frame_counts, gvtm_drift_state* d_drift,
		void* hip_stream)
{
	return generate_voice_tracks(plan, "gvtm_generate_tracks_chunks_device", VoiceEvents{d_events, d_chunk_offsets, d_voice_ids, true, d_utt_chunks}, batch,
			max_frames, d_params, d_frame_counts, d_drift, hip_stream);
}

int gvtm_synthesize_events_chunks_device(gvtm_plan* plan, const gvtm_event* d_events, const int64_t* d_chunk_offsets, const int64_t* d_utt_chunks,
		const int32_t* d_voice_ids, size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts,
		int64_t* d_out_counts, float* d_maxabs, gvtm_drift_state* d_drift, void* hip_stream)
{
	return synthesize_voice_events(plan, "gvtm_synthesize_events_chunks_device", VoiceEvents{d_events, d_chunk_offsets, d_voice_ids, true, d_utt_chunks},
			batch, max_frames, d_audio, audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift, hip_stream);
}

} // extern "C"
