// C ABI of libgama_vtm.so, rhythm and intonation points: the prosody object (the constants of intonation.txt and rhythm.txt,
// the two factors and the vocoid table, checked, copied, uploaded), the two rules on the host, for a batch on the device,
// and the prosody entry, which puts the rhythm kernel in front of gvtm_generate_events_device and the placement kernels
// between it and gvtm_apply_intonation_device, with buffers of the plan's in between.
#include <memory>

#include "vtm_host.hpp"
#include "vtm_prosody.hpp"

using namespace gvtm::host;

struct gvtm_prosody {
	int device = GVTM_DEVICE_NONE;
	gvtm_prosody_config config{};
	std::vector<uint8_t> vocoid;
	DeviceBuffer d_vocoid;
};

namespace {

bool bad_control_period(int32_t cp) { return cp < 1 || cp > 4; }

template <typename T> bool too_many(size_t n) { return n > SIZE_MAX / sizeof(T); }

// the rhythm kernel on the caller's stream (the prosody object's device is current); out of place, the postures are copied first
int launch_rhythm(const gvtm_prosody* prosody, const gvtm_posture* d_postures, const int64_t* d_posture_offsets, size_t n_postures, const gvtm_foot* d_feet,
		const int64_t* d_foot_offsets, size_t n_feet, size_t batch, gvtm_posture* d_postures_out, int32_t* d_status, hipStream_t stream)
{
	hipError_t e = hipSuccess;
	if (d_postures_out != d_postures && n_postures > 0) {
		e = hipMemcpyAsync(d_postures_out, d_postures, sizeof(gvtm_posture) * n_postures, hipMemcpyDeviceToDevice, stream);
	}
	if (e == hipSuccess && d_status) e = hipMemsetAsync(d_status, 0, sizeof(int32_t) * batch, stream);
	if (e != hipSuccess) return fail_hip(e, "rhythm: copy of the postures or clearing of the statuses");
	gvtm::ProsodyRhythmArgs args{};
	args.config = prosody->config;
	args.postures = d_postures;
	args.posture_offsets = d_posture_offsets;
	args.n_postures = static_cast<int64_t>(n_postures);
	args.feet = d_feet;
	args.foot_offsets = d_foot_offsets;
	args.n_feet = static_cast<int64_t>(n_feet);
	args.batch = batch;
	args.postures_out = d_postures_out;
	args.status = d_status;
	e = gvtm::launch_apply_rhythm(args, stream);
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "rhythm launch");
}

// what the rhythm entry and the prosody entry refuse of the rhythm's tables
int check_rhythm_tables(size_t n_postures, size_t n_feet, size_t batch)
{
	if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	if (n_postures > static_cast<size_t>(INT64_MAX) / sizeof(gvtm_posture) || n_feet > 0x7fffffffull * 256) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "n_postures or n_feet too large");
	}
	return GVTM_OK;
}

// what both placement launches hand the kernels: the object's constants and table, the caller's tables, what the rules entry left
gvtm::ProsodyPlaceArgs place_args(const gvtm_prosody* prosody, int32_t control_period, const gvtm_posture* d_postures, const int64_t* d_posture_offsets,
		const gvtm_foot* d_feet, const int64_t* d_foot_offsets, const gvtm_tone_group* d_groups, const int64_t* d_group_offsets, const double* d_draws, size_t batch,
		const gvtm_rule_data* d_rule_data, size_t max_rules, const int32_t* d_rule_counts, const double* d_onsets, gvtm_intonation_point* d_points_out,
		size_t points_capacity, int64_t* d_point_offsets_out, int32_t* d_status)
{
	gvtm::ProsodyPlaceArgs args{};
	args.config = prosody->config;
	args.vocoid = prosody->d_vocoid.as<uint8_t>();
	args.n_vocoid = static_cast<int32_t>(prosody->vocoid.size());
	args.control_period = control_period;
	args.postures = d_postures;
	args.posture_offsets = d_posture_offsets;
	args.feet = d_feet;
	args.foot_offsets = d_foot_offsets;
	args.groups = d_groups;
	args.group_offsets = d_group_offsets;
	args.draws = d_draws;
	args.batch = batch;
	args.rule_data = d_rule_data;
	args.max_rules = static_cast<int64_t>(std::min<size_t>(max_rules, INT64_MAX));
	args.rule_counts = d_rule_counts;
	args.onsets = d_onsets;
	args.points_out = d_points_out;
	args.points_capacity = static_cast<int64_t>(std::min<size_t>(points_capacity, INT64_MAX));
	args.point_offsets_out = d_point_offsets_out;
	args.status = d_status;
	return args;
}

} // namespace

extern "C" {

int gvtm_prosody_create(int device, const gvtm_prosody_config* config, const uint8_t* vocoid, size_t n_postures, gvtm_prosody** prosody_out)
{
	if (!config || !prosody_out) return fail(GVTM_ERR_INVALID_ARGUMENT, "null config or prosody_out");
	*prosody_out = nullptr;
	// (a model without the category "vocoid": the reference's UnavailableResourceException)
	if (!vocoid || n_postures == 0) return fail(GVTM_ERR_INVALID_ARGUMENT, "null or empty vocoid table: the model has no category \"vocoid\"");
	if (n_postures > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "n_postures too large");
	const char* why = gvtm::prosody_validate(*config);
	if (why[0]) return fail(GVTM_ERR_INVALID_ARGUMENT, std::string("prosody configuration: ") + why);
	if (device != GVTM_DEVICE_NONE) {
		if (const int rc = check_device_index(device, "rhythm and intonation points"); rc != GVTM_OK) return rc;
	}
	auto prosody = std::make_unique<gvtm_prosody>();
	prosody->device = device;
	prosody->config = *config;
	prosody->vocoid.assign(vocoid, vocoid + n_postures);
	if (device != GVTM_DEVICE_NONE) {
		DeviceScope scope(device);
		int rc = scope.entered();
		if (rc == GVTM_OK) rc = upload(prosody->d_vocoid, prosody->vocoid, "upload vocoid table");
		if (rc != GVTM_OK) return rc;
	}
	*prosody_out = prosody.release();
	return GVTM_OK;
}

void gvtm_prosody_destroy(gvtm_prosody* prosody)
{
	if (!prosody) return;
	if (prosody->device != GVTM_DEVICE_NONE) {
		DeviceScope scope(prosody->device); // (hipFree of the table on its device)
		delete prosody;
		return;
	}
	delete prosody;
}

int gvtm_prosody_rhythm_host(const gvtm_prosody* prosody, const gvtm_posture* postures, size_t n, const gvtm_foot* feet, size_t n_feet, gvtm_posture* postures_out,
		int32_t* status_out)
{
	if (!prosody || !status_out || (n > 0 && (!postures || !postures_out)) || (!feet && n_feet > 0)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null prosody, postures, postures_out, feet or status_out");
	}
	*status_out = gvtm::prosody_rhythm(prosody->config, postures, n, feet, n_feet, postures_out);
	return GVTM_OK;
}

int64_t gvtm_prosody_point_count(size_t n_postures, const gvtm_foot* feet, size_t n_feet, const gvtm_tone_group* groups, size_t n_groups)
{
	if ((!feet && n_feet > 0) || (!groups && n_groups > 0) || n_postures > 0x7fffffffu || n_feet > 0x7fffffffu || n_groups > 0x7fffffffu) {
		fail(GVTM_ERR_INVALID_ARGUMENT, "null feet or groups, or a table too long");
		return -1;
	}
	const int64_t count = gvtm::prosody_point_count(static_cast<int64_t>(n_postures), feet, static_cast<int64_t>(n_feet), groups, static_cast<int64_t>(n_groups));
	if (count < 0) fail(GVTM_ERR_INVALID_ARGUMENT, "feet or tone groups the reference could not have built");
	return count;
}

int gvtm_prosody_points_host(const gvtm_prosody* prosody, int32_t control_period, const gvtm_posture* postures, size_t n, const gvtm_foot* feet, size_t n_feet,
		const gvtm_tone_group* groups, size_t n_groups, const double* draws, const gvtm_rule_data* rule_data, size_t n_rules, const double* onsets,
		int32_t rule_status, gvtm_intonation_point* points_out, size_t capacity, size_t* n_points_out, int32_t* status_out)
{
	if (!prosody || !n_points_out || !status_out || (!postures && n > 0) || (!feet && n_feet > 0) || (!groups && n_groups > 0) || (!rule_data && n_rules > 0) ||
			(!onsets && n > 0)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null prosody, postures, feet, groups, rule data, onsets, n_points_out or status_out");
	}
	if (bad_control_period(control_period)) return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period must be 1..4");
	gvtm_intonation_point points[gvtm::kProsodyMaxPoints];
	const int count = gvtm::prosody_points(prosody->config, prosody->vocoid.data(), static_cast<int32_t>(prosody->vocoid.size()), control_period, postures, n, feet,
			n_feet, groups, n_groups, draws, rule_data, n_rules, n_rules, onsets, rule_status, points, status_out);
	*n_points_out = static_cast<size_t>(count);
	if (points_out && static_cast<size_t>(count) > capacity) return fail(GVTM_ERR_INVALID_ARGUMENT, "the points do not fit capacity (gvtm_prosody_point_count)");
	for (int i = 0; points_out && i < count; ++i) points_out[i] = points[i];
	return GVTM_OK;
}

int gvtm_apply_rhythm_device(const gvtm_prosody* prosody, const gvtm_posture* d_postures, const int64_t* d_posture_offsets, size_t n_postures,
		const gvtm_foot* d_feet, const int64_t* d_foot_offsets, size_t n_feet, size_t batch, gvtm_posture* d_postures_out, int32_t* d_status, void* hip_stream)
{
	if (!prosody) return fail(GVTM_ERR_INVALID_ARGUMENT, "null prosody");
	if (batch > 0 && (!d_posture_offsets || !d_foot_offsets || (n_postures > 0 && (!d_postures || !d_postures_out)) || (n_feet > 0 && !d_feet))) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null postures, posture offsets, feet, foot offsets or postures_out");
	}
	if (const int rc = check_rhythm_tables(n_postures, n_feet, batch); rc != GVTM_OK) return rc;
	if (prosody->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "prosody created with GVTM_DEVICE_NONE: host use only");
	if (batch == 0) return GVTM_OK;
	DeviceScope scope(prosody->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	return launch_rhythm(prosody, d_postures, d_posture_offsets, n_postures, d_feet, d_foot_offsets, n_feet, batch, d_postures_out, d_status,
			static_cast<hipStream_t>(hip_stream));
}

int gvtm_place_intonation_device(const gvtm_prosody* prosody, int32_t control_period, const gvtm_posture* d_postures, const int64_t* d_posture_offsets,
		const gvtm_foot* d_feet, const int64_t* d_foot_offsets, const gvtm_tone_group* d_groups, const int64_t* d_group_offsets, const double* d_draws, size_t batch,
		const gvtm_rule_data* d_rule_data, size_t max_rules, const int32_t* d_rule_counts, const double* d_onsets, gvtm_intonation_point* d_points_out,
		size_t points_capacity, int64_t* d_point_offsets_out, int32_t* d_status, void* hip_stream)
{
	if (!prosody) return fail(GVTM_ERR_INVALID_ARGUMENT, "null prosody");
	if (batch > 0 && (!d_postures || !d_posture_offsets || !d_feet || !d_foot_offsets || !d_groups || !d_group_offsets || !d_rule_data || !d_rule_counts || !d_onsets ||
			!d_points_out || !d_point_offsets_out)) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null postures, feet, groups, one of their offset tables, rule data, rule counts, onsets, points_out or point_offsets_out");
	}
	if (bad_control_period(control_period)) return fail(GVTM_ERR_INVALID_ARGUMENT, "control_period must be 1..4");
	if (batch > 0x7fffffffu) return fail(GVTM_ERR_INVALID_ARGUMENT, "batch too large for one launch");
	if (prosody->device == GVTM_DEVICE_NONE) return fail(GVTM_ERR_NO_DEVICE, "prosody created with GVTM_DEVICE_NONE: host use only");
	if (batch == 0) return GVTM_OK;
	DeviceScope scope(prosody->device);
	if (const int rc = scope.entered(); rc != GVTM_OK) return rc;
	const gvtm::ProsodyPlaceArgs args = place_args(prosody, control_period, d_postures, d_posture_offsets, d_feet, d_foot_offsets, d_groups, d_group_offsets, d_draws,
			batch, d_rule_data, max_rules, d_rule_counts, d_onsets, d_points_out, points_capacity, d_point_offsets_out, d_status);
	const hipError_t e = gvtm::launch_place_intonation(args, static_cast<hipStream_t>(hip_stream));
	return e == hipSuccess ? GVTM_OK : fail_hip(e, "intonation placement launch");
}

int gvtm_synthesize_prosody_device(gvtm_plan* plan, const gvtm_rules* rules, const gvtm_prosody* prosody, const gvtm_posture* d_postures,
		const int64_t* d_posture_offsets, size_t n_postures, const gvtm_foot* d_feet, const int64_t* d_foot_offsets, size_t n_feet, const gvtm_tone_group* d_groups,
		const int64_t* d_group_offsets, const double* d_draws, const int32_t* d_voice_ids, size_t max_rules, size_t points_capacity, size_t events_capacity,
		size_t batch, size_t max_frames, float* d_audio, size_t audio_stride, int32_t* d_frame_counts, int64_t* d_out_counts, float* d_maxabs,
		gvtm_drift_state* d_drift, int32_t* d_prosody_status, int32_t* d_status, void* hip_stream)
{
	if (!plan || !rules || !prosody) return fail(GVTM_ERR_INVALID_ARGUMENT, "null plan, rules or prosody");
	if (plan->voice_tracks.empty()) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "gvtm_synthesize_prosody_device: the plan has no track configurations yet (gvtm_plan_set_voice_tracks)");
	}
	if (plan->device == GVTM_DEVICE_NONE) return refuse_design_only();
	if (rules_device(rules) != plan->device || prosody->device != plan->device) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "the rules or the prosody object live on another device than the plan");
	}
	if (batch == 0) return GVTM_OK;
	if (!d_postures || !d_posture_offsets || !d_feet || !d_foot_offsets || !d_groups || !d_group_offsets || !d_voice_ids) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "null postures, feet, groups, one of their offset tables or voice ids");
	}
	int rc = check_rhythm_tables(n_postures, n_feet, batch);
	if (rc != GVTM_OK) return rc;
	// (what the synthesis launch would refuse is refused before any kernel writes a status)
	if (!d_audio) return fail(GVTM_ERR_INVALID_ARGUMENT, "null audio buffer");
	if ((rc = check_audio_stride(plan, audio_stride, max_frames, true)) != GVTM_OK) return rc;
	if (max_rules == 0 || too_many<gvtm_rule_data>(max_rules) || batch > SIZE_MAX / sizeof(gvtm_rule_data) / max_rules) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "max_rules is 0 or too large");
	}
	if (too_many<gvtm_intonation_point>(points_capacity) || too_many<gvtm_event>(events_capacity) ||
			points_capacity > SIZE_MAX / sizeof(gvtm_event) - events_capacity) {
		return fail(GVTM_ERR_INVALID_ARGUMENT, "points_capacity or events_capacity too large");
	}
	const size_t merged_capacity = events_capacity + points_capacity;
	DeviceScope scope(plan->device);
	if ((rc = scope.entered()) != GVTM_OK) return rc;
	auto& s = plan->async.prosody;
	struct Need { DeviceBuffer& buffer; size_t bytes; const char* what; };
	// (a buffer's pointer goes to the kernels even when there is room for nothing)
	const Need needs[] = {
		{s.postures, sizeof(gvtm_posture) * std::max<size_t>(n_postures, 1), "hipMalloc postures after rhythm"},
		{s.rhythm_status, sizeof(int32_t) * batch, "hipMalloc rhythm statuses"},
		{s.events, sizeof(gvtm_event) * std::max<size_t>(events_capacity, 1), "hipMalloc generated events"},
		{s.event_offsets, sizeof(int64_t) * (batch + 1), "hipMalloc generated event offsets"},
		{s.rule_data, sizeof(gvtm_rule_data) * batch * max_rules, "hipMalloc rule data"},
		{s.rule_counts, sizeof(int32_t) * batch, "hipMalloc rule counts"},
		{s.onsets, sizeof(double) * std::max<size_t>(n_postures, 1), "hipMalloc onsets"},
		{s.points, sizeof(gvtm_intonation_point) * std::max<size_t>(points_capacity, 1), "hipMalloc intonation points"},
		{s.point_offsets, sizeof(int64_t) * (batch + 1), "hipMalloc point offsets"},
		{s.status, sizeof(int32_t) * batch, "hipMalloc prosody statuses"},
		{s.list_ids, sizeof(int32_t) * batch, "hipMalloc list ids"},
		{plan->async.events, sizeof(gvtm_event) * std::max<size_t>(merged_capacity, 1), "hipMalloc merged events"},
		{plan->async.event_offsets, sizeof(int64_t) * (batch + 1), "hipMalloc merged event offsets"},
	};
	for (const Need& n : needs) {
		if (const hipError_t e = n.buffer.ensure(n.bytes); e != hipSuccess) return fail_hip(e, n.what);
	}
	const int32_t cp = plan->voice_tracks[0].control_period;
	hipStream_t stream = static_cast<hipStream_t>(hip_stream);
	gvtm_posture* postures = s.postures.as<gvtm_posture>();
	int32_t* prosody_status = d_prosody_status ? d_prosody_status : s.status.as<int32_t>();
	// rhythm -> postures of the plan's; the rule on them -> events, rule data and onsets of the plan's, its statuses where the
	// placement reads them and leaves its own
	rc = launch_rhythm(prosody, d_postures, d_posture_offsets, n_postures, d_feet, d_foot_offsets, n_feet, batch, postures, s.rhythm_status.as<int32_t>(), stream);
	if (rc != GVTM_OK) return rc;
	rc = gvtm_generate_events_device(rules, cp, postures, d_posture_offsets, batch, s.events.as<gvtm_event>(), events_capacity, s.event_offsets.as<int64_t>(),
			s.rule_data.as<gvtm_rule_data>(), max_rules, s.rule_counts.as<int32_t>(), s.onsets.as<double>(), prosody_status, hip_stream);
	if (rc != GVTM_OK) return rc;
	gvtm::ProsodyPlaceArgs args = place_args(prosody, cp, postures, d_posture_offsets, d_feet, d_foot_offsets, d_groups, d_group_offsets, d_draws, batch,
			s.rule_data.as<gvtm_rule_data>(), max_rules, s.rule_counts.as<int32_t>(), s.onsets.as<double>(), s.points.as<gvtm_intonation_point>(), points_capacity,
			s.point_offsets.as<int64_t>(), prosody_status);
	args.rhythm_status = s.rhythm_status.as<int32_t>();
	args.voice_k = static_cast<const gvtm::TrackConstants*>(plan->d_voice_tracks.ptr);
	args.voice_ids = d_voice_ids;
	args.n_voices = plan->n_voices();
	args.list_ids_out = s.list_ids.as<int32_t>();
	if (const hipError_t e = gvtm::launch_place_intonation(args, stream); e != hipSuccess) return fail_hip(e, "intonation placement launch");
	// the points into the lists (a refused utterance has list id -1: no list, no frames), then the lists to samples
	rc = gvtm_apply_intonation_device(plan, s.events.as<gvtm_event>(), s.event_offsets.as<int64_t>(), batch, s.list_ids.as<int32_t>(),
			s.points.as<gvtm_intonation_point>(), s.point_offsets.as<int64_t>(), d_voice_ids, batch, plan->async.events.as<gvtm_event>(), merged_capacity,
			plan->async.event_offsets.as<int64_t>(), d_status, hip_stream);
	if (rc != GVTM_OK) return rc;
	return gvtm_synthesize_events_voices_device(plan, plan->async.events.as<gvtm_event>(), plan->async.event_offsets.as<int64_t>(), d_voice_ids, batch, max_frames,
			d_audio, audio_stride, d_frame_counts, d_out_counts, d_maxabs, d_drift, hip_stream);
}

} // extern "C"
